// rtw_ahead.h — bookkeeping of k_path's reserve of camera rays and of its gated scene-bounds test (rtw_kernels.h k_path).
// Plain integer functions, constexpr so that the kernel and the host call the same code: tests/native/ahead_check.cpp simulates a wave
// over them with g++. No HIP in here.
//
// The reserve: a lane of the hot instantiation keeps up to K = RTW_PATH_AHEAD camera-ray directions of its unit's next samples in LDS,
// the entry of sample s (relative to the call's sample_offset, as k_path's s_cur) in slot s mod K. The entries are consecutive samples,
// so the only per-lane state is their count, packed into the two high bits of the lane's blk_end word (block counts stay far below
// 2^30: a pass has at most 2^28 blocks of 16 samples).
#pragma once
#include <stdint.h>

#include "../../include/rtw.h"

#ifndef RTW_PATH_AHEAD
#define RTW_PATH_AHEAD 2  // entries per lane (0: no reserve, the camera ray is generated when the lane needs it; at most 3)
#endif
#ifndef RTW_PATH_GATE_BOUNDS
#define RTW_PATH_GATE_BOUNDS 1  // 1: the scene-bounds test of camera rays runs only in iterations where it decides whether the wave walks
#endif
// The one-light instantiation (DESIGN.md 4.1 "One listed light is a compile-time fact"): 1: k_path<..., NEE1 = 1> compiles shade_a's light
// sample for exactly one listed rectangle light read from the LDS page; 0: that instantiation is the generic code (the instruction stream
// the kernel had without it)
#ifndef RTW_PATH_NEE1
#define RTW_PATH_NEE1 1
#endif
// The fixed-shape walk (DESIGN.md 4.1 "The metric scene's list shape is a compile-time fact"): 1: k_path<..., NEE1 = 1, SHAPE> walks the
// LDS lists with the shape's groups and counts compiled in (rtw_device.h walk_lds<ANY_HIT, SHAPE>); 0: those instantiations are the
// one-light instantiation's text
#ifndef RTW_PATH_SHAPE
#define RTW_PATH_SHAPE 1
#endif

namespace rtwk {

constexpr uint32_t kAheadShift = 30;
constexpr uint32_t kAheadMaxK = 3;
static_assert(RTW_PATH_AHEAD >= 0 && RTW_PATH_AHEAD <= (int)kAheadMaxK, "the count has two bits");

// the blk_end word: last block of the unit (exclusive, blocks of the pass) | entries in reserve << 30
constexpr uint32_t ahead_blk_end(uint32_t word) { return word & ((1u << kAheadShift) - 1u); }
constexpr uint32_t ahead_count(uint32_t word) { return word >> kAheadShift; }
constexpr uint32_t ahead_pushed(uint32_t word) { return word + (1u << kAheadShift); }
constexpr uint32_t ahead_popped(uint32_t word) { return word - (1u << kAheadShift); }

// first sample behind the lane's unit: block blk_end of the pass (whose first block is block0 of the call), capped by the call's samples
constexpr uint32_t ahead_unit_end(uint32_t block0, uint32_t blk_end, uint32_t spp) {
    return (block0 + blk_end) * (uint32_t)RTW_SUM_BLOCK < spp ? (block0 + blk_end) * (uint32_t)RTW_SUM_BLOCK : spp;
}
// the first sample the lane holds no entry for: a live path is sample s_cur itself, so the entries start behind it
constexpr uint32_t ahead_first_uncached(uint32_t s_cur, bool alive, uint32_t count) { return s_cur + count + (alive ? 1u : 0u); }
// the fill phase generates an entry for `first` when the ring has room and the sample belongs to the unit
constexpr bool ahead_room(uint32_t count, uint32_t k, uint32_t first, uint32_t unit_end) { return count < k && first < unit_end; }
constexpr uint32_t ahead_slot(uint32_t sample, uint32_t k) { return sample % k; }
// a lane that is about to start a camera path and has nothing in reserve: one such lane makes the wave run the fill phase
constexpr bool ahead_starved(bool busy, bool alive, uint32_t count) { return busy && !alive && count == 0u; }

// The bounds test. A wave walks the lists iff some busy lane is past depth 0 or has a camera ray that may hit the scene:
// ballot(busy && (deep || may)) != 0. With deep_ballot = ballot(busy && deep) the per-lane test `may` matters only when that is 0.
constexpr bool bounds_test_decides(unsigned long long deep_ballot) { return deep_ballot == 0ull; }

}  // namespace rtwk
