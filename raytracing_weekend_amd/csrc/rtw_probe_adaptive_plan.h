// rtw_probe_adaptive_plan.h — what one pass of rtw_probe_adaptive / rtw_probe_adaptive_device launches, decided on the host from sizes
// alone (no HIP in here, in the style of rtw_radiance_plan.h): the blocks a pass adds to every listed probe, the run of whole blocks
// that is one unit of work (R) and the units of one queue job (J), the block-sum slab in 64 bits, the cut of a list into ranges of
// list positions that fit the slab cap. The per-probe state is the adaptive family's (rtw_adaptive_plan.h, included here).
// tests/native/probe_adaptive_plan_check.cpp pins them with g++.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstddef>

#include "../../include/rtw.h"
#include "rtw_adaptive_plan.h"
#include "rtw_radiance_plan.h"

namespace rtwk {

// a pass takes every listed probe from n_from to n_to samples (both checkpoints or 0: multiples of RTW_SUM_BLOCK, n_from < n_to),
// counted from sample_offset: blocks [n_from / 16, n_to / 16) of the probe. The summation unit that block b closes is b's own,
// (b + 1) % RTW_SUM_UNIT_BLOCKS == 0, whatever sample_offset is: blocks and units are counted from it.
inline uint32_t probe_adaptive_first_block(int32_t n_from) { return (uint32_t)n_from / RTW_SUM_BLOCK; }
inline uint32_t probe_adaptive_pass_blocks(int32_t n_from, int32_t n_to) { return (uint32_t)(n_to - n_from) / RTW_SUM_BLOCK; }

// One slab entry per (block of the pass, list position): a float4 block sum. An occlusion pass keeps its uint32 count in the first
// 4 of the same 16 bytes' budget (as rtw_probe's counts do in rtw_radiance's slab).
constexpr uint64_t kProbeAdaptiveBlockBytes = 16;
inline uint64_t probe_adaptive_slab_bytes(uint64_t positions, uint32_t pass_blocks) { return positions * (uint64_t)pass_blocks * kProbeAdaptiveBlockBytes; }

// R, the whole blocks of one unit of work. Every block sum reaches memory on its own, so the blocks of a probe need no order among
// lanes and a probe's pass may be cut into as many runs as it has blocks. The cut is chosen so that the launch has about eight
// units per resident lane (`lanes`): a late pass - few probes, hundreds of samples each - still fills the device and does not end
// on one long unit, and an early pass over many probes takes each probe's blocks in one run (one list and probe fetch per run).
inline uint32_t probe_adaptive_run_blocks(uint64_t n_list, uint32_t pass_blocks, uint64_t lanes) {
    const uint64_t want = 8ull * std::max<uint64_t>(lanes, 1);                                     // units the launch should have
    const uint64_t runs = std::min<uint64_t>(pass_blocks, (want + n_list - 1) / std::max<uint64_t>(n_list, 1));  // per position, >= 1
    return (uint32_t)((pass_blocks + runs - 1) / std::max<uint64_t>(runs, 1));
}
inline uint32_t probe_adaptive_runs(uint32_t pass_blocks, uint32_t run_blocks) { return (pass_blocks + run_blocks - 1) / run_blocks; }

// list positions of one launch: as many as the slab cap holds (a position's row of pass_blocks entries stays together, so at least
// one position whatever the cap) and as one launch may number (positions * runs units, below 2^31)
inline uint64_t probe_adaptive_range_positions(uint64_t n_list, uint32_t pass_blocks, uint32_t run_blocks, uint64_t cap_bytes) {
    const uint64_t runs = probe_adaptive_runs(pass_blocks, run_blocks);
    uint64_t per = kRadianceMaxLaunchUnits / runs;
    per = std::min<uint64_t>(per, cap_bytes / ((uint64_t)pass_blocks * kProbeAdaptiveBlockBytes));
    return std::min<uint64_t>(std::max<uint64_t>(per, 1), std::max<uint64_t>(n_list, 1));
}
// (the ranges themselves are radiance_n_ranges / radiance_range over list positions)

// J: a job is 64 * j consecutive units, taken by a wave with one atomic (rtw_radiance_plan.h radiance_job_units: the same two
// rules, with a unit of 16 * R samples in the place of min(spp, 128))
inline uint32_t probe_adaptive_job_units(uint32_t run_blocks, uint64_t n_units, uint64_t waves) {
    const uint64_t per_unit = (uint64_t)run_blocks * RTW_SUM_BLOCK;
    uint64_t j = (512u + per_unit - 1u) / per_unit;
    const uint64_t balance = n_units / (64ull * std::max<uint64_t>(waves, 1) * 8ull);
    j = std::max<uint64_t>(1, std::min<uint64_t>(j, balance));
    return (uint32_t)(64ull * j);
}

}  // namespace rtwk
