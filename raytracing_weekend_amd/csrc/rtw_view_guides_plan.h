// rtw_view_guides_plan.h — what rtw_views_guides and rtw_denoise_views decide on the host from sizes alone (no HIP in here, in the
// style of rtw_radiance_plan.h): the staging of a chunk's requested guide buffers, the split of a flattened pixel into (frame, y, x)
// as k_atrous_guided_views takes it, where a denoiser pass reads and writes, and the denoiser's scratch.
// tests/native/view_guides_plan_check.cpp pins them with g++.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstddef>

#include "../../include/rtw.h"
#include "rtw_radiance_plan.h"
#include "rtw_stage_plan.h"

namespace rtwk {

// bytes of one entry of rtw_guides' buffers, in the struct's order: albedo, normal (float4), depth (float), prim (int32)
constexpr uint64_t kGuideEntryBytes[4] = {16, 16, 4, 4};

// The staging of one chunk of the host entry, inside the query family's staging slab (rtw_stage_plan.h stage_plan over the four entry
// sizes): the requested buffers one after another, each 256-byte aligned; a buffer nobody asked for takes nothing. off[k] is valid
// where want[k].
struct ViewGuideStage { uint64_t off[4]; uint64_t bytes; };
inline ViewGuideStage view_guides_stage(uint64_t chunk, const bool want[4]) {
    const StagePlan p = stage_plan(chunk, 4, kGuideEntryBytes, want);
    return ViewGuideStage{{p.off[0], p.off[1], p.off[2], p.off[3]}, p.bytes};
}
// pixels of one chunk: all of them, or as many as RTW_RADIANCE_CHUNK says (at least 1)
inline uint64_t view_guides_chunk(uint64_t n, uint64_t knob) { return std::min<uint64_t>(std::max<uint64_t>(n, 1), std::max<uint64_t>(knob, 1)); }

// pixel p of n_views frames of width x height: its frame's first pixel, its row and its column (what k_atrous_guided_views computes
// with magic_div's constants of width * height), and the address of tap (dx, dy) * step clamped to the frame
struct FramePixel { uint64_t base; int32_t y, x; };
inline FramePixel frame_pixel(uint64_t p, int32_t width, int32_t height) {
    const ViewPixel v = view_pixel(p, width, height);
    return FramePixel{v.view * (uint64_t)(uint32_t)width * (uint64_t)(uint32_t)height, (int32_t)v.y, (int32_t)v.x};
}
inline uint64_t frame_tap(const FramePixel& f, int32_t width, int32_t height, int32_t dx, int32_t dy, int32_t step) {
    const int64_t yy = std::min<int64_t>(std::max<int64_t>((int64_t)f.y + (int64_t)dy * step, 0), (int64_t)height - 1);
    const int64_t xx = std::min<int64_t>(std::max<int64_t>((int64_t)f.x + (int64_t)dx * step, 0), (int64_t)width - 1);
    return f.base + (uint64_t)(yy * (int64_t)width + xx);
}

// a frame of rtw_denoise_views is a frame rtw_denoise_guided takes: at most 2^28 pixels (width, height > 0), so that a tap's
// x + 2 * 128 and y * width + x stay ints in the kernel
inline bool denoise_views_frame_ok(int32_t width, int32_t height) { return (int64_t)width * (int64_t)height <= ((int64_t)1 << 28); }

// The passes of rtw_denoise_views alternate between the output and one scratch buffer so that the last pass writes the output: pass
// `it` of `iterations` writes the output when an even number of passes follows it. Pass 0 reads the input, pass it > 0 what pass
// it - 1 wrote. The output aliases no input, so no pass reads what it writes.
inline bool denoise_views_writes_output(int32_t iterations, int32_t it) { return ((iterations - 1 - it) & 1) == 0; }
// bytes of a buffer of n pixels, 256-byte aligned
inline uint64_t denoise_views_buffer_bytes(uint64_t n) { return (n * 16ull + 255ull) & ~255ull; }
// the context's scratch: the device entry needs the one ping-pong buffer (none for a single pass); the host entry the colour, the two
// guides and the output beside it
inline uint64_t denoise_views_scratch_bytes(uint64_t n, int32_t iterations, bool host) {
    return denoise_views_buffer_bytes(n) * ((iterations > 1 ? 1ull : 0ull) + (host ? 4ull : 0ull));
}

}  // namespace rtwk
