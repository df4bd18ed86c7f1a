// CPU check of the launch planning (raytracing_weekend_amd/csrc/rtw_plan.h), compiled and run by tests/test_plan_cpu.py.
// Every choice that sets a render's speed - k_path's unit sizes, sum slots, passes and launches; the wavefront pipeline's batch
// size, lanes, trace workgroup and tail schedule - is arithmetic on sizes: the plans of a few renders are pinned here.
// usage: plan_check   (prints one line per case; exit status 0 when every check holds)
#include <cstdio>
#include <cstdlib>

#include "../../raytracing_weekend_amd/csrc/rtw_plan.h"
using namespace rtwk;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static const char* kKnobs[] = {"RTW_POOL_PATHS", "RTW_LANES", "RTW_GRID_MULT", "RTW_TAIL_START", "RTW_FUSED", "RTW_SPLIT_MEDIA", "RTW_TRACE_BLOCK",
                               "RTW_TRACE_LDS_KB", "RTW_TRACE_WAVES", "RTW_TAIL_GROUP", "RTW_STAGGER", "RTW_PATH_JOB_BLOCKS", "RTW_PATH_UNIT_BLOCKS",
                               "RTW_PATH_FINE_BLOCKS", "RTW_PATH_GRID_MULT", "RTW_BLOCKSUM_BYTES"};
// the tuning a render reads with `name=value` set (nullptr: the defaults)
static Tuning tuning(const char* name = nullptr, const char* value = nullptr) {
    for (const char* k : kKnobs) unsetenv(k);
    if (name) setenv(name, value, 1);
    const Tuning t = read_tuning();
    if (name) unsetenv(name);
    return t;
}

static void print_path(const char* what, const PathPlan& p) {
    printf("path %s: blocks %zu U %zu F %zu unit_sums %d passes %zu (of %zu blocks) slots %zu\n", what, p.n_blocks, p.U, p.F, (int)p.unit_sums,
           p.passes.size(), p.pass_blocks, p.need_slots);
}
static void print_wave(const char* what, const WavefrontPlan& w) {
    printf("wavefront %s: S %zu lanes %d grid_mult %u stagger %d trace %d threads / %zu B / grid %d regions %u x %zu steps %zu\n", what, w.S,
           w.n_lanes, w.grid_mult, w.stagger_pct, w.trace_block, w.trace_lds, w.trace_grid, w.regions_max, w.region_cap_max, w.sched.size());
}

int main() {
    const size_t hd = 1920 * 1080;
    // a 4-wide tree like scene 1's (240 nodes), 16-bit stack entries
    const SceneFacts tree{true, 0, 240, 300, 21, false};
    const SceneFacts lists{false, 0, 0, 0, 0, false};

    {   // the headline: 1920x1080, 4096 spp, 256 CUs, 6 k_path workgroups per CU
        const PathPlan p = plan_path(tuning(), hd, 4096, 256, 6);
        print_path("headline", p);
        CHECK(p.n_blocks == 256 && p.n_groups == 32400 && p.U == 8 && p.F == 8 && p.unit_sums);
        CHECK(p.passes.size() == 1 && p.pass_blocks == 256 && p.need_slots == 39 && !p.too_many_jobs);
        const PathPass& ps = p.passes[0];
        CHECK(ps.b0 == 0 && ps.nb == 256 && ps.nb_coarse == 248 && ps.slots_coarse == 31);
        const PathLaunch& bulk = ps.part[0];
        CHECK(bulk.first == 0 && bulk.count == 248 && bulk.unit_blocks == 8 && bulk.jb == 2 && bulk.n_ranges == 16 && bulk.n_jobs == 518400 && bulk.grid == 1536);
        const PathLaunch& fine = ps.part[1];
        CHECK(fine.first == 248 && fine.count == 8 && fine.unit_blocks == 1 && fine.jb == 2 && fine.n_ranges == 4 && fine.n_jobs == 129600 && fine.grid == 1536);
    }
    {   // 256 spp on the same frame: 84 blocks per lane, 4-block units, a pass that short is all fine units
        const PathPlan p = plan_path(tuning(), hd, 256, 256, 6);
        print_path("256spp", p);
        CHECK(p.n_blocks == 16 && p.U == 4 && p.F == 16 && !p.unit_sums && p.passes.size() == 1 && p.need_slots == 16);
        const PathPass& ps = p.passes[0];
        CHECK(ps.nb_coarse == 0 && ps.slots_coarse == 0 && ps.part[0].count == 0);
        CHECK(ps.part[1].count == 16 && ps.part[1].unit_blocks == 1 && ps.part[1].n_ranges == 8 && ps.part[1].n_jobs == 259200 && ps.part[1].grid == 1536);
    }
    {   // BASELINE config 5: 7680x4320, 4096 spp - 39 slots would not fit the 16 GiB block-sum cap (32 slots): two passes
        const PathPlan p = plan_path(tuning(), (size_t)7680 * 4320, 4096, 256, 6);
        print_path("c5", p);
        CHECK(p.U == 8 && p.F == 8 && p.unit_sums && p.pass_blocks == 200 && p.need_slots == 32 && p.passes.size() == 2);
        CHECK(p.passes[0].b0 == 0 && p.passes[0].nb == 200 && p.passes[0].nb_coarse == 192 && p.passes[0].slots_coarse == 24);
        CHECK(p.passes[1].b0 == 200 && p.passes[1].nb == 56 && p.passes[1].nb_coarse == 48 && p.passes[1].slots_coarse == 6);
        CHECK(p.passes[1].part[0].n_ranges == 3 && p.passes[1].part[0].n_jobs == 518400 * 3 && p.passes[1].part[1].n_jobs == 518400 * 4);
    }
    {   // RTW_BLOCKSUM_BYTES: room for 24 slots of the headline frame - the pass search stops at the first size past the cap, and
        // 32 blocks (all fine units, 32 slots) is past it: passes of 24 blocks -, then for one slot of a small frame (passes never go
        // below one summation unit of 8 blocks)
        char v[32];
        snprintf(v, sizeof v, "%zu", 24 * hd * 16);
        PathPlan p = plan_path(tuning("RTW_BLOCKSUM_BYTES", v), hd, 4096, 256, 6);
        print_path("blocksum24", p);
        CHECK(p.pass_blocks == 24 && p.passes.size() == 11 && p.need_slots == 24 && p.passes[10].b0 == 240 && p.passes[10].nb == 16);
        CHECK(p.passes[0].nb_coarse == 0 && p.passes[0].part[1].count == 24);
        p = plan_path(tuning("RTW_BLOCKSUM_BYTES", "65536"), 64 * 64, 256, 256, 6);
        print_path("blocksum64k", p);
        CHECK(p.pass_blocks == 8 && p.passes.size() == 2 && p.need_slots == 8 && !p.unit_sums && p.passes[1].b0 == 8);
    }
    {   // knobs: unit and fine sizes; grid capped by the jobs of a small frame
        const PathPlan p = plan_path(tuning("RTW_PATH_UNIT_BLOCKS", "16"), 64 * 64, 4096, 256, 6);
        print_path("unit16", p);
        CHECK(p.U == 16 && p.F == 8 && p.unit_sums && p.passes[0].nb_coarse == 240 && p.passes[0].part[0].n_ranges == 8);
        CHECK(p.passes[0].part[0].n_jobs == 64 * 8 && p.passes[0].part[0].grid == 128);
    }

    {   // BASELINE config 3 on scene 1: 1920x1080, 512 spp, two lanes, the default pool (2^30 paths): two equal batches of 256
        const WavefrontPlan w = plan_wavefront(tuning(), hd, 512, 0, 50, ~(size_t)0, 256, tree);
        print_wave("c3", w);
        CHECK(w.S == 256 && w.n_lanes == 2 && w.grid_mult == 4 && w.stagger_pct == 0);
        CHECK(w.batch_size(0, 0) == 256 && w.batch_size(1, 256) == 256);
        CHECK(w.regions_max == 1024 && w.region_cap_max == (2025 + 2) * 256 && w.cnt_words == (size_t)1024 * (w.sched.size() + 2));
        // every node in LDS: 512-thread workgroups, two per CU (5 waves per SIMD)
        CHECK(w.trace_block == 512 && w.trace_nodes == 240 && w.trace_leaves == 0 && w.trace_grid == 256 * 2);
        // split pipeline to bounce 20, then the tail in groups of 2, 2, 3, 3, 4, 4, 6, 6 bounces
        CHECK(w.split_first && w.sched.size() == 38 + 8);
        CHECK(w.sched[0].kind == RTW_K_TRACE && w.sched[0].depth == 1 && w.sched[1].kind == RTW_K_SHADE && w.sched[37].depth == 19);
        const int tail[8][2] = {{20, 2}, {22, 2}, {24, 3}, {27, 3}, {30, 4}, {34, 4}, {38, 6}, {44, 6}};
        for (int k = 0; k < 8; k++)
            CHECK(w.sched[38 + k].kind == RTW_K_BOUNCE && w.sched[38 + k].depth == tail[k][0] && w.sched[38 + k].n_iter == tail[k][1]);
    }
    {   // a smaller pool: 2^28 paths, 8 batches of 64
        const WavefrontPlan w = plan_wavefront(tuning("RTW_POOL_PATHS", "268435456"), hd, 512, 0, 50, ~(size_t)0, 256, tree);
        print_wave("pool2^28", w);
        CHECK(w.S == 64 && w.n_lanes == 2);
        // the device's own limit (pool_cap, halved after a failed allocation) counts the same way
        CHECK(plan_wavefront(tuning(), hd, 512, 0, 50, (size_t)1 << 28, 256, tree).S == 64);
    }
    {   // three lanes, a pool of 2e7 paths on 640x480 at 100 spp: 21 samples fit, 6 equal batches of 17; the candidate-list
        // scene's lanes start a third and two thirds of a batch late; no tree, so no trace plan
        const WavefrontPlan w = plan_wavefront(tuning("RTW_LANES", "3"), 640 * 480, 100, 0, 12, 20000000, 256, lists);
        print_wave("lanes3", w);
        CHECK(w.S == 17 && w.n_lanes == 3 && w.grid_mult == 4 && w.stagger_pct == 50);
        CHECK(w.batch_size(0, 0) == 17 && w.batch_size(1, 17) == 12 && w.batch_size(2, 29) == 6 && w.batch_size(3, 35) == 17 && w.batch_size(7, 97) == 3);
        CHECK(w.trace_lds == 0 && w.trace_grid == 0 && w.trace_block == 256);
        // depth 12: the split pipeline to bounce 6 (k_first has done bounce 0), then tail groups of 2, 2, 2
        CHECK(w.sched.size() == 13 && w.sched[10].depth == 6 && w.sched[10].n_iter == 2 && w.sched[12].depth == 10 && w.sched[12].n_iter == 2);
    }
    {   // samples_per_pass given: no equal-batch rounding; one lane when one batch holds all samples
        WavefrontPlan w = plan_wavefront(tuning(), hd, 512, 100, 50, ~(size_t)0, 256, tree);
        CHECK(w.S == 100 && w.n_lanes == 2);
        w = plan_wavefront(tuning(), 64 * 64, 8, 0, 6, ~(size_t)0, 256, lists);
        print_wave("small", w);
        CHECK(w.S == 4 && w.n_lanes == 2 && w.regions_max == 64 && w.region_cap_max == 3 * 256);
        w = plan_wavefront(tuning("RTW_LANES", "1"), 64 * 64, 8, 0, 6, ~(size_t)0, 256, lists);
        CHECK(w.S == 8 && w.n_lanes == 1 && w.grid_mult == 8);
    }
    {   // media: tail from 40 on; RTW_FUSED: every bounce through k_bounce, depth 0 included
        const SceneFacts media{true, 1, 1419, 2000, 30, false};
        WavefrontPlan w = plan_wavefront(tuning(), hd, 256, 0, 50, ~(size_t)0, 256, media);
        CHECK(w.split_first && w.sched.size() == 78 + 4 && w.sched[78].depth == 40 && w.sched[81].depth == 47 && w.sched[81].n_iter == 3);
        CHECK(w.trace_block == 256 && w.trace_nodes < 1419 && w.trace_lds <= 16 * 1024);
        w = plan_wavefront(tuning("RTW_FUSED", "1"), hd, 256, 0, 8, ~(size_t)0, 256, lists);
        CHECK(!w.split_first && w.sched.size() == 6 + 1 && w.sched[0].kind == RTW_K_BOUNCE && w.sched[0].depth == 0 && w.sched[6].n_iter == 2);
    }
    {   // exact division constants
        const uint32_t ds[] = {1, 2, 3, 7, 640, 1920, 7680, 65535};
        for (uint32_t d : ds) {
            uint32_t m, s1, s2;
            magic_div(d, m, s1, s2);
            for (uint32_t n : {0u, 1u, d - 1u, d, 12345678u, 0xfffffffeu, 0xffffffffu}) {
                const uint32_t t = (uint32_t)(((uint64_t)m * n) >> 32);
                CHECK(((((n - t) >> s1) + t) >> s2) == n / d);
            }
        }
    }
    if (fails) fprintf(stderr, "%d checks failed\n", fails);
    return fails ? 1 : 0;
}
