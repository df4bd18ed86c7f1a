// rtw_plan.h — what a render launches, decided on the host from sizes alone: the tuning knobs, the k_path passes and launches
// (plan_path) and the wavefront pipeline's batches, trace workgroup and schedule (plan_wavefront). No HIP in here: rtw_hip.hip's
// issue_path_pass / run_batches issue what these plans say, for every renderer, and tests/native/plan_check.cpp pins them with g++.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <vector>

#include "../../include/rtw.h"
#include "rtw_bvh.h"

namespace rtwk {

constexpr int kBlock = 256;                       // 4 wave64 per workgroup
#ifndef RTW_MAX_REGIONS
#define RTW_MAX_REGIONS 1024
#endif
// 1 024 regions = 4 compacting workgroups per CU (what two lanes use; a single lane used to take 8). Round 3 halved the table: it is
// static LDS of every wavefront kernel (4 KB instead of 8), and LDS is what decides whether the other lane's workgroups find room
// on a CU beside a resident k_trace_bvh (scene 4 +5 %, scene 1 +2 %).
constexpr uint32_t kMaxRegions = RTW_MAX_REGIONS;            // region counters scanned in LDS by every workgroup (>= the compacting grid)
constexpr uint32_t kSumBlock = RTW_SUM_BLOCK;
constexpr uint32_t kSumUnitBlocks = RTW_SUM_UNIT_BLOCKS;
constexpr int kPathMaxPrims = 64;  // k_path walks the brute lists only: scenes of at most this many primitives
constexpr int kBruteMaxPrims = 24;  // at or below: scalar-cache brute lists; above: BVH with the LDS stack

// multiply-high constants for exact 32-bit division by an invariant d >= 1 (Granlund & Montgomery 1994)
inline void magic_div(uint32_t d, uint32_t& m, uint32_t& s1, uint32_t& s2) {
    uint32_t l = 0;
    while (l < 32 && ((uint64_t)1 << l) < d) l++;
    m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << l) - d)) / d + 1);
    s1 = l < 1 ? l : 1;
    s2 = l > 0 ? l - 1 : 0;
}

// Tuning knobs, read from the environment once per call site (defaults are what profiles/ was measured with):
//   RTW_POOL_PATHS  paths in flight over all lanes (default 2^30: sized for 288 GB of HBM - a full-HD frame at 512+ spp takes 178 GB of
//                   state without listed lights, 238 GB with; an allocation that fails is halved, see render_wavefront. Round 3, BASELINE
//                   config 3: 2^28 (8 batches of 64 spp) 6.7, 2^29 (4 x 128) 7.0, 2^30 (2 x 256) 7.3 Gsamples/s)
//   RTW_LANES       stream lanes that overlap consecutive batches (default 2; 1..4)
//   RTW_GRID_MULT   persistent workgroups per CU (default 8 with one lane, 4 with two)
//   RTW_TAIL_START  first bounce handled by the fused multi-bounce tail launches (default 6; 20 for tree scenes, 40 for tree scenes with media)
//   RTW_FUSED=1     every bounce through the fused k_bounce
//   RTW_SPLIT_MEDIA=0  scenes with media: every bounce through k_bounce (default: split pipeline, volumes tested in the shading kernels)
//   RTW_BRUTE_MAX   largest primitive count walked with the scalar-cache brute lists (default 24; 0 forces the BVH)
//   RTW_LDS_KB      dynamic LDS per workgroup for traversal stacks + staged tree nodes (default 16)
//   RTW_TAIL_GROUP  bounces per launch of the first tail group (default 2; groups grow by half every second launch)
//   RTW_FIRST_GROUP_LOG2  k_first: 2^n neighbouring threads start samples of one pixel (default 3; 0 = one sample of 64 pixels per wave)
//   RTW_STAGGER     how far the second lane starts behind the first, in percent of a batch (its first batch is cut short by that
//                   much; 0 = no offset). Default: 50 for the candidate-list scenes under RTW_PATH=0, 0 for tree scenes (there the
//                   extra batch costs more than the offset gains: scenes 1, 2, 4 +1-4 % at 512+ spp, +6-13 % at 128-256 spp)
//   RTW_PATH        1 (default): scenes walked with the brute lists render through k_path (paths in registers, in-wave
//                   regeneration); 0: always the wavefront pipeline
//   RTW_PATH_UNIT_BLOCKS 16-sample blocks a lane takes as one unit in the bulk launch (default: 8 = 128 samples when a lane has
//                        600+ blocks to do, else 4)
//   RTW_PATH_FINE_BLOCKS blocks at the end of a pass that a second, concurrent launch hands out one by one (default: 8 behind 8-block
//                        units, 16 behind shorter ones)
//   RTW_PATH_JOB_BLOCKS  units per pixel in one k_path job (default 2: a job is 64 pixels x 2 units)
//   RTW_PATH_GRID_MULT   k_path workgroups per CU (default: what the occupancy query admits)
//   RTW_BLOCKSUM_BYTES   cap of the k_path block-sum buffer (default 16 GiB); larger renders run in passes over the samples
//   RTW_KERNEL_TIMING    0: no per-launch events even when the caller asks for rtw_stats (kernel_seconds stay 0)
//   RTW_CULL             0: k_path is handed every 64-pixel group, also those no camera ray of which can reach a primitive (default 1:
//                        such groups get no job and their pixels are black, see cull_rect below; same image and counts either way)
//   RTW_CAST_CHUNK       rays rtw_cast (the host variant) stages and casts at a time (default 2^20: 76 MB of staging at all five outputs;
//                        1 .. 2^31 - 1). The results do not depend on it.
//   RTW_CAST_GRID_MULT   k_cast workgroups per CU (default: what the occupancy query admits, the persistent launch; larger values queue
//                        workgroups behind the resident ones - for measurements). The results do not depend on it.
//   RTW_RADIANCE_CHUNK   rays rtw_radiance (the host variant) stages and traces at a time (default 2^20: 48 MB of staging; 1 .. 2^31 - 1).
//                        Chunk c runs with the stream key of its first ray: the results do not depend on it.
//   RTW_RADIANCE_SLAB_BYTES  cap of rtw_radiance's unit-sum slab (calls beyond 128 spp: 16 B per ray and 128 samples; default 1 GiB). A
//                        larger batch runs as consecutive ray ranges (csrc/rtw_radiance_plan.h). The results do not depend on it.
//   RTW_PATHS_CHUNK_BYTES  what rtw_paths / rtw_paths_views (the host variants) stage of heads and records at a time (default 256 MiB; at
//                        least 1): a chunk is the most whole rays that fit, and at least one (csrc/rtw_paths_plan.h). Chunk c runs with
//                        the stream key of its first ray: the results do not depend on it.
// Two measured-slower alternatives were removed from the code: k_path_tree for tree scenes and the paired batch
// schedule; their knobs are no longer read.
struct Tuning {
    size_t pool_paths = (size_t)1 << 30;
    int lanes = 2;
    int grid_mult = 0;   // 0 = automatic
    int tail_start = 0;  // 0 = automatic: 6 for the brute-list scenes, 20 for tree scenes (40 with media)
    bool fused = false;
    bool split_media = true;  // RTW_SPLIT_MEDIA=0: scenes with media keep every bounce in k_bounce
    int brute_max = kBruteMaxPrims;
    size_t lds_kb = 16;
    int trace_block = 256;       // threads per workgroup of k_trace_bvh (256, 512, 1024)
    size_t trace_lds_kb = 16;    // its LDS budget: stacks + tree nodes + leaf records
    bool trace_auto = true;      // neither RTW_TRACE_BLOCK nor RTW_TRACE_LDS_KB given: the render picks the pair (see plan_wavefront)
    int trace_waves = 5;         // waves per SIMD it is launched for (the kernel is compiled for 6: 78 VGPRs). 5 leaves a SIMD the 96 VGPRs of one
                                 // wave of the other lane's k_shade; medians of 5 renders, 6 -> 5 -> 4: scene 1 7 242 / 7 285 / 7 072 Msamples/s,
                                 // scene 2 3 593 / 3 664 / 3 646, scene 4 2 123 / 2 128 / 2 059 (profiles/r03_trace_waves_sweep.txt)
    int stagger_pct = -1;  // -1 = automatic
    int tail_group = 2;
    int first_group_log2 = 3;    // k_first: up to 2^this neighbouring threads take samples of one pixel (RTW_FIRST_GROUP_LOG2; round 2: 16;
                                 // round 3, with the wave-coherent walk: 8 (scene 1 medians of 5: 7 085 against 6 948-6 998 Msamples/s; 4: 7 091;
                                 // 2: 7 066; 1: 7 011; scenes 2 and 4 do not care). Round 2's note on 16:
                                 // k_first -6 ... -14 %; at 64 the later launches lose more - their finished paths then write
                                 // 16-byte results npix apart - than k_first gains)
    int path = 1;
    int path_job_blocks = 2;
    int path_unit_blocks = 0;    // 0 = automatic (8 for large renders, else 4)
    int path_fine_blocks = -1;   // -1 = automatic (8 behind 8-block units, 16 behind shorter ones)
    int path_grid_mult = 0;
    size_t blocksum_bytes = (size_t)16 << 30;
    bool kernel_timing = true;
    bool cull = true;
    size_t cast_chunk = (size_t)1 << 20;  // rtw_cast: rays per staged chunk
    int cast_grid_mult = 0;               // k_cast workgroups per CU; 0 = the occupancy query's answer
    size_t radiance_chunk = (size_t)1 << 20;        // rtw_radiance: rays per staged chunk
    size_t radiance_slab_bytes = (size_t)1 << 30;   // rtw_radiance: cap of the unit-sum slab
    size_t paths_chunk_bytes = (size_t)256 << 20;   // rtw_paths: heads and records per staged chunk
    bool verbose = false;  // RTW_VERBOSE=1: table sizes at upload (stderr)
};
inline Tuning read_tuning() {
    Tuning t;
    auto geti = [](const char* name, long long& out) {
        const char* e = getenv(name);
        if (!e || !*e) return false;
        out = atoll(e);
        return true;
    };
    long long v;
    if (geti("RTW_POOL_PATHS", v) && v >= 1024) t.pool_paths = (size_t)v;
    if (geti("RTW_LANES", v)) t.lanes = (int)std::max<long long>(1, std::min<long long>(4, v));
    if (geti("RTW_GRID_MULT", v)) t.grid_mult = (int)std::max<long long>(1, v);
    if (geti("RTW_TAIL_START", v)) t.tail_start = (int)std::max<long long>(1, v);
    if (geti("RTW_FUSED", v)) t.fused = v == 1;
    if (geti("RTW_SPLIT_MEDIA", v)) t.split_media = v != 0;
    if (geti("RTW_BRUTE_MAX", v)) t.brute_max = (int)v;
    if (geti("RTW_LDS_KB", v)) t.lds_kb = (size_t)std::max<long long>(0, v);
    if (geti("RTW_TRACE_BLOCK", v) && (v == 256 || v == 512 || v == 1024)) { t.trace_block = (int)v; t.trace_auto = false; }
    if (geti("RTW_TRACE_LDS_KB", v)) { t.trace_lds_kb = (size_t)std::max<long long>(0, std::min<long long>(150, v)); t.trace_auto = false; }
    if (geti("RTW_TRACE_WAVES", v)) t.trace_waves = (int)std::max<long long>(1, std::min<long long>(8, v));
    if (geti("RTW_TAIL_GROUP", v)) t.tail_group = (int)std::max<long long>(1, std::min<long long>(64, v));
    if (geti("RTW_FIRST_GROUP_LOG2", v)) t.first_group_log2 = (int)std::max<long long>(0, std::min<long long>(8, v));
    if (geti("RTW_STAGGER", v)) t.stagger_pct = (int)std::max<long long>(0, std::min<long long>(99, v));
    if (geti("RTW_PATH", v)) t.path = (int)std::max<long long>(0, std::min<long long>(2, v));
    if (geti("RTW_PATH_JOB_BLOCKS", v)) t.path_job_blocks = (int)std::max<long long>(1, std::min<long long>(1024, v));
    if (geti("RTW_PATH_UNIT_BLOCKS", v)) t.path_unit_blocks = (int)std::max<long long>(0, std::min<long long>(4096, v));
    if (geti("RTW_PATH_FINE_BLOCKS", v)) t.path_fine_blocks = (int)std::max<long long>(-1, std::min<long long>(4096, v));
    if (geti("RTW_PATH_GRID_MULT", v)) t.path_grid_mult = (int)std::max<long long>(1, std::min<long long>(16, v));
    if (geti("RTW_BLOCKSUM_BYTES", v) && v >= (1 << 16)) t.blocksum_bytes = (size_t)v;
    if (geti("RTW_KERNEL_TIMING", v)) t.kernel_timing = v != 0;
    if (geti("RTW_CULL", v)) t.cull = v != 0;
    if (geti("RTW_CAST_CHUNK", v)) t.cast_chunk = (size_t)std::max<long long>(1, std::min<long long>(0x7fffffffll, v));
    if (geti("RTW_CAST_GRID_MULT", v)) t.cast_grid_mult = (int)std::max<long long>(0, std::min<long long>(4096, v));
    if (geti("RTW_RADIANCE_CHUNK", v)) t.radiance_chunk = (size_t)std::max<long long>(1, std::min<long long>(0x7fffffffll, v));
    if (geti("RTW_RADIANCE_SLAB_BYTES", v)) t.radiance_slab_bytes = (size_t)std::max<long long>(16, v);
    if (geti("RTW_PATHS_CHUNK_BYTES", v)) t.paths_chunk_bytes = (size_t)std::max<long long>(1, v);
    if (geti("RTW_VERBOSE", v)) t.verbose = v != 0;
    return t;
}

// LDS of a tree-walking workgroup of `block` threads: the traversal stacks (16-bit entries unless a reference needs more),
// then as many leading (breadth-first) tree nodes and, once all nodes are in, leaf records as fit `budget` bytes.
inline size_t tree_lds_layout(size_t n_nodes_all, size_t n_leaves_all, int stack_depth, bool wide, size_t block, size_t budget, int32_t& n_nodes,
                              int32_t& n_leaves) {
    const size_t stack_words = wide ? (size_t)stack_depth * block : ((size_t)stack_depth * block + 1) / 2;
    const size_t stack_bytes = ((stack_words + 3) & ~size_t(3)) * 4;
    size_t room = budget > stack_bytes ? budget - stack_bytes : 0;
    n_nodes = (int32_t)std::min<size_t>(n_nodes_all, room / sizeof(rtwbvh::Q4Node));
    room -= (size_t)n_nodes * sizeof(rtwbvh::Q4Node);
    n_leaves = (size_t)n_nodes == n_nodes_all ? (int32_t)std::min<size_t>(n_leaves_all, room / sizeof(rtwbvh::LeafRec)) : 0;
    return stack_bytes + (size_t)n_nodes * sizeof(rtwbvh::Q4Node) + (size_t)n_leaves * sizeof(rtwbvh::LeafRec);
}

// ---- k_path: paths in registers, lanes regenerate; only the unit sums (16 B per pixel and 64 samples) reach HBM
// One launch of a pass: `count` blocks from block `first` of the pass, handed out in units of `unit_blocks` blocks, `jb` units per
// pixel and job; n_jobs = 64-pixel groups x n_ranges.
struct PathLaunch { size_t first, count, unit_blocks, jb, n_ranges, n_jobs; int grid; };
// A pass over blocks [b0, b0 + nb): the bulk launch (part[0]: coarse units) and the end-game launch on the second stream (part[1]:
// single-block units); a launch whose count is 0 is not issued.
struct PathPass { size_t b0, nb, nb_coarse, slots_coarse; PathLaunch part[2]; };
struct PathPlan {
    size_t n_blocks, n_groups, U, F, pass_blocks, need_slots;
    bool unit_sums;
    bool too_many_jobs;  // some launch would have more jobs than the queue counts
    std::vector<PathPass> passes;
};

// live_groups: the groups that get jobs (cull_live_groups; default: all of them). It sets the job count and the grid; the unit size
// keeps following the full pixel count (blocks_per_lane below), so a culled render is planned like the uncut one with fewer jobs.
inline PathPlan plan_path(const Tuning& tune, size_t npix, int spp, int n_cu, int wg_per_cu, size_t live_groups = ~(size_t)0) {
    PathPlan p{};
    const size_t n_blocks = ((size_t)spp + kSumBlock - 1) / kSumBlock;
    const size_t n_groups = (npix + 63) / 64;
    live_groups = std::min(live_groups, n_groups);
    p.n_blocks = n_blocks;
    p.n_groups = n_groups;
    // A launch ends when its slowest unit ends, and a unit through a glass sphere runs several milliseconds. So the bulk of
    // a pass is handed out in units of `unit_blocks` blocks (one lane keeps a pixel for 64 samples: little bookkeeping), and
    // its last `fine_blocks` blocks in single-block units by a SECOND launch on a second stream: its workgroups move into the
    // slots the first launch's workgroups vacate as they run dry, so the machine stays full until only 16-sample units are
    // left (measured on the 1/8 shard of the metric frame: see DESIGN.md section 6).
    // Unit size: every unit costs a little (queue, camera-ray set-up, a 16-byte store per block either way) and a launch
    // ends with its longest units, so long renders want long units and short ones short units. Measured on the metric
    // frame (1 620 blocks per lane): 8-block units 0.556 s, 4-block 0.562 s, 2-block 0.581 s; on its 1/8 shard (202
    // blocks per lane): 0.0773, 0.0722, 0.0736 s; on the 1/2 shard 8 and 4 are level.
    const size_t blocks_per_lane = npix * n_blocks / ((size_t)n_cu * (size_t)wg_per_cu * kBlock);
    const size_t U = tune.path_unit_blocks > 0 ? (size_t)tune.path_unit_blocks : (blocks_per_lane >= 600 ? 8 : 4);
    // the end-game region: the last 8 blocks of a pass behind 8-block units, the last 16 behind 4-block units (a shard-sized
    // render: the bulk launch drains for a unit's length at its end, and the single-block work beside it must last that long;
    // 1/8 shard of the metric frame, medians of 12 runs: F = 8 0.0739 s, 16 0.0725, 24 0.0728, 32 0.0727, 48 0.0729; the full
    // frame does not care: 0.5597 against 0.5593)
    const size_t F = tune.path_fine_blocks >= 0 ? (size_t)tune.path_fine_blocks : (U >= 8 ? 8 : 16);
    // Sums in memory (the arithmetic spec's three levels, rtw.h): a bulk launch whose lane units are whole summation units
    // (U a multiple of 8 blocks) stores ONE float4 per unit and pixel, everything else one per block; k_resolve_blocks adds
    // them up in the spec's order. A pass covers a multiple of 8 blocks, so no summation unit straddles two passes.
    const bool unit_sums = (U % kSumUnitBlocks) == 0;
    auto coarse_of = [&](size_t nb) { return nb > 4 * F ? ((nb - F) / U) * U : (size_t)0; };  // short passes are all fine units
    auto slots_of = [&](size_t nb) { const size_t nc = coarse_of(nb); return unit_sums ? nc / kSumUnitBlocks + (nb - nc) : nb; };
    const size_t cap_slots = std::max<size_t>(1, tune.blocksum_bytes / (npix * 16));  // 16: a float4 sum per slot and pixel
    size_t pass_blocks = n_blocks;
    if (slots_of(n_blocks) > cap_slots) {
        pass_blocks = kSumUnitBlocks;
        while (pass_blocks + kSumUnitBlocks < n_blocks && slots_of(pass_blocks + kSumUnitBlocks) <= cap_slots) pass_blocks += kSumUnitBlocks;
    }
    size_t need_slots = 0;
    for (size_t b0 = 0; b0 < n_blocks; b0 += pass_blocks) need_slots = std::max(need_slots, slots_of(std::min(pass_blocks, n_blocks - b0)));
    p.U = U; p.F = F; p.unit_sums = unit_sums; p.pass_blocks = pass_blocks; p.need_slots = need_slots;
    for (size_t b0 = 0; b0 < n_blocks; b0 += pass_blocks) {
        PathPass ps{};
        ps.b0 = b0;
        ps.nb = std::min(pass_blocks, n_blocks - b0);
        ps.nb_coarse = coarse_of(ps.nb);
        ps.slots_coarse = unit_sums ? ps.nb_coarse / kSumUnitBlocks : ps.nb_coarse;
        for (int part = 0; part < 2; part++) {
            PathLaunch& l = ps.part[part];
            l.first = part == 0 ? 0 : ps.nb_coarse;
            l.count = part == 0 ? ps.nb_coarse : ps.nb - ps.nb_coarse;
            if (l.count == 0) continue;
            l.unit_blocks = part == 0 ? U : 1;
            const size_t n_units = (l.count + l.unit_blocks - 1) / l.unit_blocks;    // units per pixel in this launch
            l.jb = std::min<size_t>((size_t)tune.path_job_blocks, n_units);        // units per pixel and job
            l.n_ranges = (n_units + l.jb - 1) / l.jb;
            l.n_jobs = live_groups * l.n_ranges;
            if (l.n_jobs > 0xfffffff0ull) p.too_many_jobs = true;
            l.grid = (int)std::min<size_t>((size_t)n_cu * (size_t)wg_per_cu, (l.n_jobs + 3) / 4);
        }
        p.passes.push_back(ps);
    }
    return p;
}

// ---- pixels that certainly see nothing (k_path renders of scenes without a sky light: DESIGN.md 4.1)
// A camera ray that meets no primitive adds +0 to its pixel when the scene has no sky light, so a pixel none of whose rays can
// meet one is black without being traced. cull_bounds: world bounds of every primitive, generous enough for the float arithmetic of
// the primitive tests; cull_rect: the pixel rectangle outside which every pixel is certainly empty; cull_group_live /
// cull_live_groups: the 64-pixel groups of a shard that have a pixel inside it (k_classify drops the others from the job order
// with the same integer predicate; k_path itself knows nothing of this).
struct CullRect { int32_t x0, x1, y0, y1; };  // every pixel outside [x0, x1) x [y0, y1) (full-image coordinates) is certainly empty

// Union of the primitives' world bounds (rtw_bvh.h world_bounds: the reference's boxes + 1e-4 relative), spheres grown by what their
// discriminant can get wrong: fma(b, b, -(a * cc)) carries an error of a few 2^-23 |o - c|^2 |d|^2, so a ray passing the centre at
// distance m can be reported as a hit while m^2 < r^2 + ~2^-21 |o - c|^2. They are grown to sqrt(r^2 + 2^-19 D^2), D = |o - c| + r in
// object space, times the transform's Frobenius norm. Returns false (nothing may be culled) when there is no primitive, a moving
// sphere (a ray time outside the sphere's own keys moves it out of its swept box) or something not finite.
inline bool cull_bounds(const rtw_prim* prims, size_t n_prims, const rtw_xform* xforms, const rtw_camera& cam, float bmin[3], float bmax[3]) {
    rtwbvh::Box all;
    for (size_t i = 0; i < n_prims; i++) {
        const rtw_prim& p = prims[i];
        const rtw_xform& xf = xforms[p.xform];
        if (p.type == RTW_PRIM_MOVING_SPHERE) return false;
        rtwbvh::Box wb = rtwbvh::world_bounds(p, xf);
        if (p.type == RTW_PRIM_SPHERE || p.type == RTW_PRIM_VOLUME_SPHERE) {
            double oo[3], frob = 0.0, grow = 0.0;
            for (int a = 0; a < 3; a++) oo[a] = (double)xf.inv[4 * a] * cam.origin[0] + (double)xf.inv[4 * a + 1] * cam.origin[1] + (double)xf.inv[4 * a + 2] * cam.origin[2] + xf.inv[4 * a + 3];
            for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) frob += (double)xf.m[4 * a + b] * xf.m[4 * a + b];
            const double r = std::fabs((double)p.p[3]);
            const float* c = p.p;
            const double D = std::sqrt((oo[0] - c[0]) * (oo[0] - c[0]) + (oo[1] - c[1]) * (oo[1] - c[1]) + (oo[2] - c[2]) * (oo[2] - c[2])) + r;
            grow = std::sqrt(r * r + D * D / 524288.0) - r;
            const float g = (float)(grow * std::sqrt(frob) * 1.000001);
            for (int a = 0; a < 3; a++) { wb.mn[a] -= g; wb.mx[a] += g; }
        }
        all.add(wb);
    }
    bool ok = n_prims > 0;
    for (int a = 0; a < 3; a++) {
        bmin[a] = all.mn[a]; bmax[a] = all.mx[a];
        ok = ok && std::isfinite(bmin[a]) && std::isfinite(bmax[a]) && bmin[a] <= bmax[a];
    }
    return ok;
}

// The rectangle for a frame of width x height pixels. raygen (rtw_kernels.h) builds d = lower_left + s horizontal + t vertical - origin
// with s = (x + r0) / width, t = (y + r1) / height, r in [0, 1): pixel (x, y) covers s in [x, x + 1] / width ((float)x + r0 may round up
// to x + 1), t likewise. The eight corners of the bounds, grown by 2^-13 of the largest coordinate around (bounds and camera origin: the
// primitive tests' float error is some 2^-20 of it), are projected onto (s, t) in double precision: corner - origin = a horizontal +
// b vertical + c (lower_left - origin), s = a / c, t = b / c. With every c > 0 the bounds' projection is the convex hull of the eight
// points, inside their bounding rectangle. That rectangle is widened to whole pixels and by ONE MORE pixel on every side, which pays for
// the rounding of raygen's own arithmetic: s and the two fused multiply-adds and the subtraction leave component k of d off by at most
// eps_k = 4 * 2^-24 max(|origin_k|, |lower_left_k| + |horizontal_k| + |vertical_k|), which moves (s, t) by at most err_s, err_t computed
// below - the rectangle is only used when both are below half a pixel (else: whole frame). Whole frame also for a sky light, any camera
// but the perspective one without a lens, a corner not strictly in front of the camera, a singular camera frame, anything not finite.
inline CullRect cull_rect(const rtw_camera& cam, int cam_type, int sky_light, const float bmin[3], const float bmax[3], int width, int height) {
    const CullRect whole{0, width, 0, height};
    if (sky_light != 0 || cam_type != RTW_CAM_PERSPECTIVE || cam.lens_radius != 0.0f || width <= 0 || height <= 0) return whole;
    double m[3][3], big = 0.0, eps[3];  // columns: horizontal, vertical, lower_left - origin
    for (int a = 0; a < 3; a++) {
        m[a][0] = cam.horizontal[a]; m[a][1] = cam.vertical[a]; m[a][2] = (double)cam.lower_left[a] - (double)cam.origin[a];
        if (!(bmin[a] <= bmax[a])) return whole;
        big = std::max(big, std::max(std::fabs((double)bmin[a]), std::max(std::fabs((double)bmax[a]), std::fabs((double)cam.origin[a]))));
        eps[a] = std::max(std::fabs((double)cam.origin[a]), std::fabs((double)cam.lower_left[a]) + std::fabs(m[a][0]) + std::fabs(m[a][1])) * (4.0 / 16777216.0);
        if (!std::isfinite(eps[a])) return whole;
    }
    if (!std::isfinite(big)) return whole;
    double inv[3][3];
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    if (!std::isfinite(det) || det == 0.0) return whole;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const int r0 = (j + 1) % 3, r1 = (j + 2) % 3, c0 = (i + 1) % 3, c1 = (i + 2) % 3;  // inv[i][j] = cofactor(j, i) / det
            inv[i][j] = (m[r0][c0] * m[r1][c1] - m[r0][c1] * m[r1][c0]) / det;
        }
    // raygen's rounding: a direction error e moves s = a / c (c = 1 on the image plane) by |inv_a e - s inv_c e|, |s| <= 1 + a pixel
    double err_s = 0.0, err_t = 0.0;
    for (int k = 0; k < 3; k++) {
        err_s += (std::fabs(inv[0][k]) + 1.01 * std::fabs(inv[2][k])) * eps[k];
        err_t += (std::fabs(inv[1][k]) + 1.01 * std::fabs(inv[2][k])) * eps[k];
    }
    if (!(err_s * width <= 0.5 && err_t * height <= 0.5)) return whole;
    const double pad = big / 8192.0;
    double smin = HUGE_VAL, smax = -HUGE_VAL, tmin = HUGE_VAL, tmax = -HUGE_VAL, cmin = HUGE_VAL, cmax = 0.0;
    for (int k = 0; k < 8; k++) {
        double q[3], abc[3];
        for (int a = 0; a < 3; a++) q[a] = (((k >> a) & 1) ? (double)bmax[a] + pad : (double)bmin[a] - pad) - (double)cam.origin[a];
        for (int i = 0; i < 3; i++) abc[i] = inv[i][0] * q[0] + inv[i][1] * q[1] + inv[i][2] * q[2];
        if (!(abc[2] > 0.0)) return whole;
        cmin = std::min(cmin, abc[2]); cmax = std::max(cmax, abc[2]);
        smin = std::min(smin, abc[0] / abc[2]); smax = std::max(smax, abc[0] / abc[2]);
        tmin = std::min(tmin, abc[1] / abc[2]); tmax = std::max(tmax, abc[1] / abc[2]);
    }
    if (!(cmin > 1.0e-6 * cmax) || !std::isfinite(smin) || !std::isfinite(smax) || !std::isfinite(tmin) || !std::isfinite(tmax)) return whole;
    auto lo = [](double v, int n) { return (int32_t)std::max(0.0, std::min((double)n, std::floor(v * n) - 1.0)); };
    auto hi = [](double v, int n) { return (int32_t)std::max(0.0, std::min((double)n, std::floor(v * n) + 2.0)); };
    CullRect r{lo(smin, width), hi(smax, width), lo(tmin, height), hi(tmax, height)};
    if (r.x0 >= r.x1 || r.y0 >= r.y1) r = CullRect{0, 0, 0, 0};  // the frame looks past everything
    return r;
}

// Group g of a shard: its shard-local pixels [64 g, 64 g + 64) below npix, local pixel p at x = p % width, y = row0 + (p / width) row_stride.
// Live = one of them lies inside the rectangle. k_classify decides the same with the same integers (one pixel per lane, a ballot).
inline bool cull_group_live(const CullRect& r, size_t g, size_t npix, uint32_t width, uint32_t row0, uint32_t row_stride) {
    const size_t p0 = g * 64, p1 = std::min(npix, p0 + 64);
    for (size_t yl = p0 / width; yl * width < p1; yl++) {
        const int64_t y = (int64_t)row0 + (int64_t)(yl * row_stride);
        if (y < r.y0 || y >= r.y1) continue;
        const int64_t xa = (int64_t)(std::max(p0, yl * width) - yl * width), xb = (int64_t)(std::min(p1, (yl + 1) * width) - yl * width);  // [xa, xb)
        if (xa < r.x1 && xb > r.x0) return true;
    }
    return false;
}
// live groups of the shard and (culled_pixels) the pixels of the others: those k_path never sees
inline size_t cull_live_groups(const CullRect& r, size_t npix, uint32_t width, uint32_t row0, uint32_t row_stride, size_t* culled_pixels = nullptr) {
    const size_t n_groups = (npix + 63) / 64;
    size_t live = 0, dead_pix = 0;
    if (npix == 0 || width == 0) { if (culled_pixels) *culled_pixels = 0; return 0; }
    if (r.x0 <= 0 && r.y0 <= 0 && r.x1 >= (int64_t)width && (int64_t)row0 + (int64_t)((npix + width - 1) / width - 1) * row_stride < r.y1) live = n_groups;  // nothing culled
    else
        for (size_t g = 0; g < n_groups; g++) {
            if (cull_group_live(r, g, npix, width, row0, row_stride)) live++;
            else dead_pix += std::min(npix, g * 64 + 64) - g * 64;
        }
    if (culled_pixels) *culled_pixels = dead_pix;
    return live;
}

// ---- wavefront pipeline (tree scenes; RTW_PATH=0)
// what of the uploaded scene the plan looks at
struct SceneFacts {
    bool use_bvh;
    int n_vol;
    size_t n_tree_nodes, n_tree_leaves;  // 4-wide nodes and leaf records of the tree
    int stack_depth;
    bool stack_wide;
};
// Launch schedule of one batch. Wide bounces: one k_shade + one k_trace per bounce (split pipeline; scenes
// whose intersection programs draw random numbers keep trace and shade fused in k_bounce instead).
// Thin tail: k_bounce with several bounces in registers, in growing groups. kind: RTW_K_TRACE, RTW_K_SHADE or RTW_K_BOUNCE.
struct Step { int kind, depth, n_iter; };
struct WavefrontPlan {
    size_t S;             // samples per pixel of a full batch
    int spp, n_lanes, n_cu, stagger_pct;
    uint32_t grid_mult;
    int trace_block;      // k_trace_bvh (tree scenes): workgroup size, LDS image, grid
    size_t trace_lds;
    int32_t trace_nodes, trace_leaves;
    int trace_grid;
    uint32_t regions_max;
    size_t region_cap_max, cnt_words;
    std::vector<Step> sched;
    bool split_first;     // k_first traces and shades depth 0 itself (split pipeline)

    // Persistent compacting grid: G workgroups (8 per CU when a lane has the GPU to itself, 4 when two lanes share it).
    // Output region b belongs to workgroup b, which is handed every G-th 256-path chunk of its input: at most
    // ceil(chunks / G) + 1 chunks (the work list of a later launch has up to one partial chunk per region more than
    // the first), so a region of (ceil(chunks / G) + 2) * 256 slots cannot overflow.
    uint32_t grid_for(size_t paths) const {
        const size_t chunks = (paths + kBlock - 1) / kBlock;
        return (uint32_t)std::min<size_t>(std::min<size_t>(chunks, (size_t)n_cu * grid_mult), (size_t)kMaxRegions);
    }
    size_t cap_for(size_t paths) const {
        const size_t chunks = (paths + kBlock - 1) / kBlock;
        const size_t g = grid_for(paths);
        return ((chunks + g - 1) / g + 2) * (size_t)kBlock;
    }
    // samples of batch b, which starts at sample s0
    size_t batch_size(size_t b, size_t s0) const {
        size_t want = S;
        if (stagger_pct > 0 && b > 0 && b < (size_t)n_lanes && S > 1)  // lane k starts k/n_lanes of a batch late (at 50 %)
            want = std::max<size_t>(1, S - S * b * (size_t)stagger_pct * 2 / (100 * (size_t)n_lanes));
        return std::min(want, (size_t)spp - s0);
    }
};

inline WavefrontPlan plan_wavefront(const Tuning& tune, size_t npix, int spp, int samples_per_pass, int max_depth, size_t pool_cap, int n_cu,
                                    const SceneFacts& sf) {
    WavefrontPlan w{};
    w.spp = spp;
    w.n_cu = n_cu;
    // samples per pass: keep about pool_target paths in flight, split over the lanes
    const int want_lanes = tune.lanes;
    size_t S = samples_per_pass > 0 ? (size_t)samples_per_pass : std::max<size_t>(1, std::min(tune.pool_paths, pool_cap) / (size_t)want_lanes / npix);
    S = std::min<size_t>(S, (size_t)spp);
    while (S > 1 && npix * S > 0xfffffff0ull) S--;
    if (samples_per_pass <= 0 && want_lanes > 1 && (size_t)spp >= (size_t)want_lanes) {
        // equal batches, as many as a multiple of the lanes: every lane gets the same number of batches of the same size (a
        // render of 128 spp whose pool would take it in one batch would leave the second lane idle; 512 spp in batches of 129
        // would end with a short fourth one). Sizes are kept multiples of 16 where that fits (k_first's sample grouping).
        size_t nb = ((size_t)spp + S - 1) / S;
        nb = (nb + (size_t)want_lanes - 1) / (size_t)want_lanes * (size_t)want_lanes;
        size_t s_eq = ((size_t)spp + nb - 1) / nb;
        if (((s_eq + 15) & ~(size_t)15) <= S) s_eq = (s_eq + 15) & ~(size_t)15;
        S = std::max<size_t>(1, std::min(S, s_eq));
    }
    w.S = S;
    const size_t paths_max = npix * S;
    const size_t n_batches = ((size_t)spp + S - 1) / S;
    w.n_lanes = (int)std::min<size_t>((size_t)want_lanes, std::max<size_t>(n_batches, 1));
    w.grid_mult = tune.grid_mult > 0 ? (uint32_t)tune.grid_mult : (w.n_lanes > 1 ? 4u : 8u);
    // The second lane's first batch is cut short so that the lanes run half a batch apart: one lane's bandwidth-bound
    // k_shade launches then meet the other's issue-bound k_first / k_trace instead of its own kind (5 runs each on one
    // box: 9.35-9.58 Gsamples/s with the offset, 8.93-9.59 without).
    w.stagger_pct = tune.stagger_pct >= 0 ? tune.stagger_pct : (sf.use_bvh ? 0 : 50);
    // k_trace_bvh: large workgroups share one LDS copy of the tree (nodes, then leaf records) between more waves
    int trace_block = tune.trace_block;
    size_t trace_budget = tune.trace_lds_kb * 1024;
    // LDS the trace launch may plan with per CU: all 160 KB when the knobs say so; 142 KB when the render chooses - the other
    // lane's kernels (k_shade: 9 KB per workgroup) must find room beside a resident k_trace_bvh, or the two lanes take turns
    size_t trace_cu_lds = (size_t)160 * 1024;
    if (sf.use_bvh && tune.trace_auto) {
        // Every node of the tree in the workgroup's LDS image takes the global loads - and the vmcnt waits behind them - out of the
        // walk loop (k_trace_bvh mode 2), but only pays while the kernel keeps its waves AND leaves the other lane room: a 256-thread
        // workgroup at 6 per CU has 14 KB for stacks + nodes (scene 1's stacks alone: 21 levels = 10.75 KB), a 512-thread workgroup
        // shares one image between twice the waves. Measured (round 3, scene 1: 240 nodes = 15.4 KB; k_trace_bvh per 512-spp render):
        // 256 threads / 16 KB (88 nodes in LDS, the old default) 0.152-0.155 s; 256 / 26 KB (all nodes, 4 waves per SIMD) 0.154;
        // 512 / 37 KB (all nodes, 3 workgroups = 141 KB per CU) 0.144-0.147; 512 / 40.5 KB (152 KB per CU: no room left for the
        // other lane's workgroups) 0.155; 512 / 43 KB (three planned, two fit) 0.166; 512 / 44 KB (two planned) 0.143-0.145.
        // Scene 2: 0.163 -> 0.153. Scene 4 (1 419 nodes = 91 KB) stays at 256 / 16 KB.
        const size_t cu_lds = (size_t)142 * 1024;
        const size_t blocks[2] = {256, 512};
        for (size_t blk : blocks) {
            int32_t nn = 0, nl = 0;
            const size_t want = std::max<size_t>(1, (size_t)(4 * tune.trace_waves) / (blk / 64));  // workgroups per CU at the wanted occupancy
            const size_t fixed = (kMaxRegions + 1 + blk) * 4 + 64;                                // the work list's static LDS
            // stacks + every node, no leaf records (a partial leaf image makes a wave run both of leaf_test's fetch paths)
            const size_t need = tree_lds_layout(sf.n_tree_nodes, 0, sf.stack_depth, sf.stack_wide, blk, (size_t)150 * 1024, nn, nl);
            if ((size_t)nn != sf.n_tree_nodes) continue;
            const size_t fit = cu_lds / (need + fixed);
            if (fit >= want || (blk == 512 && fit >= 2)) { trace_block = (int)blk; trace_budget = need; trace_cu_lds = cu_lds; break; }
        }
    }
    w.trace_block = trace_block;
    if (sf.use_bvh) {
        w.trace_lds = tree_lds_layout(sf.n_tree_nodes, sf.n_tree_leaves, sf.stack_depth, sf.stack_wide, (size_t)trace_block, trace_budget,
                                      w.trace_nodes, w.trace_leaves);
        const size_t per_wg = w.trace_lds + (kMaxRegions + 1 + (size_t)trace_block) * 4 + 64;
        const size_t by_lds = std::max<size_t>(1, trace_cu_lds / per_wg);
        const size_t by_waves = std::max<size_t>(1, (size_t)(4 * tune.trace_waves) / ((size_t)trace_block / 64));
        w.trace_grid = (int)((size_t)n_cu * std::min(by_lds, by_waves));
    }
    w.regions_max = w.grid_for(paths_max);
    w.region_cap_max = w.cap_for(paths_max);
    // the fused tail kernel walks the tree one lane per path (lane utilisation 0.2): tree scenes stay in the split
    // pipeline longer, and longest where media keep many paths alive deep (scene 4, 3.9 segments per sample: 20 -> 40
    // +5 %; scenes 1 and 2, 2.6 and 3.2: best at 20, -2 % at 30)
    const int tail_start = tune.tail_start > 0 ? tune.tail_start : (sf.use_bvh ? (sf.n_vol > 0 ? 40 : 20) : 6);
    const bool split = !tune.fused && (sf.n_vol == 0 || tune.split_media);
    int d = 0, grp = tune.tail_group, rep = 0;
    while (d < max_depth) {
        if (d < tail_start) {
            if (split) {
                // k_first has already traced and shaded depth 0
                if (d > 0) { w.sched.push_back({RTW_K_TRACE, d, 1}); w.sched.push_back({RTW_K_SHADE, d, 1}); }
            } else {
                w.sched.push_back({RTW_K_BOUNCE, d, 1});
            }
            d++;
        } else {
            const int n = std::min(grp, max_depth - d);
            if (++rep == 2) { rep = 0; grp += grp / 2; }
            w.sched.push_back({RTW_K_BOUNCE, d, n});
            d += n;
        }
    }
    // a batch must not end with probes still queued: a zero-bounce k_bounce resolves them and retires the zombies
    if (split && (w.sched.empty() || w.sched.back().kind == RTW_K_SHADE)) w.sched.push_back({RTW_K_BOUNCE, max_depth, 0});
    w.split_first = split;
    w.cnt_words = (size_t)w.regions_max * (w.sched.size() + 2);
    return w;
}


// ---- adaptive sampling (rtw.h rtw_render_adaptive): the checkpoints n_0 = min_spp, n_{k+1} = min(cap, n_k + step), step = step_spp
// or, when step_spp is 0, n_k / 2 rounded up to a multiple of kSumBlock. A function of the three numbers alone. Returns nullptr and
// fills `out` when the settings are valid, else what is wrong with them.
inline const char* adaptive_checkpoints(int min_spp, int step_spp, int cap, float threshold, int dilate, std::vector<int>& out) {
    out.clear();
    if (cap <= 0 || cap % (int)kSumBlock != 0) return "the cap (params->spp) must be a positive multiple of RTW_SUM_BLOCK";
    if (min_spp < 2 * (int)kSumBlock || min_spp % (int)kSumBlock != 0) return "min_spp must be a multiple of RTW_SUM_BLOCK, at least 2 * RTW_SUM_BLOCK";
    if (min_spp > cap) return "min_spp above the cap";
    if (step_spp < 0 || step_spp % (int)kSumBlock != 0) return "step_spp must be 0 or a positive multiple of RTW_SUM_BLOCK";
    if (!(threshold >= 0.0f)) return "threshold must be >= 0 (NaN is not)";
    if (dilate != 0 && dilate != 1) return "dilate must be 0 or 1";
    for (long long n = min_spp;;) {
        out.push_back((int)n);
        if (n >= cap) break;
        const long long half = (n / 2 + kSumBlock - 1) / kSumBlock * kSumBlock;
        n = std::min<long long>(cap, n + (step_spp > 0 ? step_spp : half));
    }
    return nullptr;
}

}  // namespace rtwk
