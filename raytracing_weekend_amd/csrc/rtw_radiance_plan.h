// rtw_radiance_plan.h — what rtw_radiance / rtw_radiance_device launch, decided on the host from sizes alone (no HIP in here, in the
// style of rtw_plan.h): summation units per ray, the unit-sum slab in 64 bits, the cut of a batch into ray ranges that fit a slab cap,
// the stream keys of a range or chunk (they wrap modulo 2^32) and the size of the jobs a wave takes from the queue.
// tests/native/radiance_check.cpp pins them with g++.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstddef>

#include "../../include/rtw.h"

namespace rtwk {

constexpr uint32_t kRadianceUnit = RTW_SUM_BLOCK * RTW_SUM_UNIT_BLOCKS;  // samples of one summation unit: what a lane owns at a time
// units one launch may hold: unit numbers, job starts and the unit-major index u = unit * n + ray stay below 2^31 in the kernel
constexpr uint64_t kRadianceMaxLaunchUnits = 0x7fffffffull;

// summation units of one ray: ceil(spp / 128); spp > 0
inline uint32_t radiance_units(int32_t spp) { return ((uint32_t)spp + kRadianceUnit - 1u) / kRadianceUnit; }

// bytes of the slab [unit][ray] of float4 unit sums for n rays (0 when the lane writes the mean itself: one unit per ray)
inline uint64_t radiance_slab_bytes(uint64_t n, int32_t spp) {
    const uint64_t u = radiance_units(spp);
    return u <= 1 ? 0ull : n * u * 16ull;
}

// rays of one launch: as many as the slab cap holds (a ray's units stay together, so at least one ray whatever the cap) and as
// one launch may number
inline uint64_t radiance_range_rays(uint64_t n, int32_t spp, uint64_t cap_bytes) {
    const uint64_t u = radiance_units(spp);
    uint64_t rays = kRadianceMaxLaunchUnits / u;
    if (u > 1) rays = std::min<uint64_t>(rays, cap_bytes / (u * 16ull));
    return std::min<uint64_t>(std::max<uint64_t>(rays, 1), std::max<uint64_t>(n, 1));
}

// rtw_probe_sh keeps nine float4 - 144 bytes - per point and unit where a radiance query keeps one: the same three rules at that
// size. A launch's float4 index (unit * n + point) * 9 + j stays below 2^31 as well, hence a ninth of the units per launch.
constexpr uint64_t kProbeShUnitBytes = 9ull * 16ull;
constexpr uint64_t kProbeShMaxLaunchUnits = kRadianceMaxLaunchUnits / 9ull;
inline uint64_t probe_sh_slab_bytes(uint64_t n, int32_t spp) {
    const uint64_t u = radiance_units(spp);
    return u <= 1 ? 0ull : n * u * kProbeShUnitBytes;
}
inline uint64_t probe_sh_range_points(uint64_t n, int32_t spp, uint64_t cap_bytes) {
    const uint64_t u = radiance_units(spp);
    uint64_t points = kProbeShMaxLaunchUnits / u;
    if (u > 1) points = std::min<uint64_t>(points, cap_bytes / (u * kProbeShUnitBytes));
    return std::min<uint64_t>(std::max<uint64_t>(points, 1), std::max<uint64_t>(n, 1));
}

// rtw_views numbers the pixels of a call (view * height + y) * width + x and runs them as a radiance query's rays: the same units,
// slab, ranges and jobs over n = n_views * width * height, which has to stay a launch's ray count. The product is taken in 64 bits
// and by division, so that no n_views, however large, wraps it (width, height > 0).
inline bool view_pixels_ok(uint64_t n_views, int32_t width, int32_t height) {
    const uint64_t frame = (uint64_t)(uint32_t)width * (uint64_t)(uint32_t)height;
    return n_views == 0 || (frame <= kRadianceMaxLaunchUnits && n_views <= kRadianceMaxLaunchUnits / frame);
}
inline uint64_t view_pixels(uint64_t n_views, int32_t width, int32_t height) { return n_views * (uint64_t)(uint32_t)width * (uint64_t)(uint32_t)height; }
// pixel p of the flattened index: its view, row and column, and its stream key width * y + x (what the kernel computes with
// magic_div's constants for width and width * height)
struct ViewPixel { uint64_t view; uint32_t y, x, key; };
inline ViewPixel view_pixel(uint64_t p, int32_t width, int32_t height) {
    const uint64_t frame = (uint64_t)(uint32_t)width * (uint64_t)(uint32_t)height;
    const uint64_t view = p / frame;
    const uint32_t key = (uint32_t)(p - view * frame);
    return ViewPixel{view, key / (uint32_t)width, key % (uint32_t)width, key};
}

// range r of the cut of [0, n) into ranges of `per` rays: [first, first + count); count = 0 past the end
struct RadianceRange { uint64_t first, count; };
inline uint64_t radiance_n_ranges(uint64_t n, uint64_t per) { return (n + per - 1) / per; }
inline RadianceRange radiance_range(uint64_t n, uint64_t per, uint64_t r) {
    const uint64_t first = std::min<uint64_t>(r * per, n);
    return RadianceRange{first, std::min<uint64_t>(per, n - first)};
}

// stream key of the first ray of a range or chunk that starts at ray `first`: ray i draws from key_offset + i modulo 2^32
inline uint32_t radiance_key(uint32_t key_offset, uint64_t first) { return (uint32_t)((uint64_t)key_offset + first); }

// Units of one job: 64 * J consecutive units, taken by a wave with one atomic on the queue word. An agent-scope atomic costs
// ~0.4 us and atomics on one address serialise (rtw_kernels.h, "Stream compaction without global atomics"): the queue serves at
// most ~2.5 M jobs/s. The kernel shades up to 22 G segments/s (profiles/radiance_rates.txt) and a unit is at least min(spp, 128)
// segments, so J with 64 * J * min(spp, 128) >= 32 768 keeps the queue below 0.7 M jobs/s - about a quarter of what it can serve -
// in the worst case (every path one segment): J = 512 / min(spp, 128), 4 at 128 spp and beyond, 512 at spp 1. Small batches take
// smaller jobs, so that the resident waves (`waves`) each see about eight jobs and the launch does not end on one long job; never
// less than one unit per lane. That second rule wins on the full-HD frames of the rates file: J = 1 at 64 spp (32 400 jobs in
// 22.5 ms on scene 0: 1.4 M jobs/s, over half of what the queue serves; a wave fetches eight times per launch and waits well under
// a microsecond each time) and J = 4 at 1024 spp (64 800 jobs in 0.23 s: 0.28 M jobs/s). DESIGN.md 4.9.
inline uint32_t radiance_job_units(int32_t spp, uint64_t n_units, uint64_t waves) {
    const uint32_t per_unit = std::min<uint32_t>((uint32_t)spp, kRadianceUnit);
    uint64_t j = (512u + per_unit - 1u) / per_unit;
    const uint64_t balance = n_units / (64ull * std::max<uint64_t>(waves, 1) * 8ull);
    j = std::max<uint64_t>(1, std::min<uint64_t>(j, balance));
    return (uint32_t)(64ull * j);
}
inline uint64_t radiance_n_jobs(uint64_t n_units, uint32_t job_units) { return (n_units + job_units - 1) / job_units; }

}  // namespace rtwk
