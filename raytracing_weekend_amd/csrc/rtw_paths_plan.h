// rtw_paths_plan.h — how the host variants of rtw_paths / rtw_paths_views cut a call into chunks of whole rays (pixels), decided on
// the host from sizes alone (no HIP in here, in the style of rtw_radiance_plan.h). A ray's samples stay together: a chunk holds the
// most whole rays whose heads and records fit the budget (RTW_PATHS_CHUNK_BYTES, rtw_plan.h), and at least one. Offsets are 64-bit:
// 2^31 - 1 pairs of up to 2^20 records of 64 bytes stay below 2^57. tests/native/paths_plan_check.cpp pins it with g++.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/rtw.h"

namespace rtwk {

constexpr uint64_t kPathsMaxPairs = 0x7fffffffull;  // (ray, sample) pairs of one call: a launch numbers them in 32 bits

// n * spp stays a launch's pair count; by division, so that no n wraps the product (spp > 0)
inline bool paths_pairs_ok(uint64_t n, int32_t spp) { return n == 0 || n <= kPathsMaxPairs / (uint64_t)(uint32_t)spp; }

// bytes of one ray's results: spp heads and spp * K records
inline uint64_t paths_ray_bytes(int32_t spp, int32_t K) {
    return (uint64_t)(uint32_t)spp * (sizeof(rtw_path_head) + (uint64_t)(uint32_t)K * sizeof(rtw_path_vertex));
}

// The cut of [0, n) into chunks of `rays` rays, the last one shorter.
struct PathsPlan { uint64_t rays, n_chunks; };
inline PathsPlan paths_plan(uint64_t n, int32_t spp, int32_t K, uint64_t chunk_bytes) {
    const uint64_t rays = std::min<uint64_t>(std::max<uint64_t>(chunk_bytes / paths_ray_bytes(spp, K), 1), std::max<uint64_t>(n, 1));
    return PathsPlan{rays, (n + rays - 1) / rays};
}

// chunk c of the cut: rays [first, first + count) (count = 0 past the end), and where its heads and records begin in the caller's
// arrays, in bytes
struct PathsChunk { uint64_t first, count, head_off, vertex_off; };
inline PathsChunk paths_chunk(uint64_t n, int32_t spp, int32_t K, const PathsPlan& pl, uint64_t c) {
    const uint64_t first = std::min<uint64_t>(c * pl.rays, n);
    const uint64_t pairs = first * (uint64_t)(uint32_t)spp;
    return PathsChunk{first, std::min<uint64_t>(pl.rays, n - first), pairs * sizeof(rtw_path_head),
                      pairs * (uint64_t)(uint32_t)K * sizeof(rtw_path_vertex)};
}

}  // namespace rtwk
