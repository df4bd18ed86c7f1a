// CPU check of rtw_probe_adaptive's planning (raytracing_weekend_amd/csrc/rtw_probe_adaptive_plan.h), compiled with
// g++ -fsanitize=address,undefined and run by tests/test_probe_adaptive_cpu.py: the blocks of every pass tile the probe's samples,
// the runs of R blocks tile a pass, the ranges under a slab cap tile the list, nothing wraps at 2^31 - 1 probes, and J and R never
// give zero work or more units than a launch may number; and the adaptive family's state layout (rtw_adaptive_plan.h), with and without
// the renderer's `part`. Prints "probe_adaptive_plan_check ok" and returns 0, or says what failed.
#include <cstdio>
#include <vector>

#include "../../raytracing_weekend_amd/csrc/rtw_plan.h"
#include "../../raytracing_weekend_amd/csrc/rtw_probe_adaptive_plan.h"
using namespace rtwk;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static const unsigned long long kBig = 0x7fffffffull;

// one pass over n_list positions with `lanes` resident lanes under a slab cap: R, the runs, J and the ranges
static void pass(uint64_t n_list, int32_t n_from, int32_t n_to, uint64_t lanes, uint64_t cap) {
    const uint32_t nb = probe_adaptive_pass_blocks(n_from, n_to), b0 = probe_adaptive_first_block(n_from);
    CHECK(nb >= 1 && (uint64_t)b0 * RTW_SUM_BLOCK == (uint64_t)n_from && ((uint64_t)b0 + nb) * RTW_SUM_BLOCK == (uint64_t)n_to);
    const uint32_t R = probe_adaptive_run_blocks(n_list, nb, lanes);
    CHECK(R >= 1 && R <= nb);
    const uint32_t runs = probe_adaptive_runs(nb, R);
    CHECK(runs >= 1 && (uint64_t)runs * R >= nb && (uint64_t)(runs - 1) * R < nb);  // the runs tile the pass, the last one not empty
    // enough units to fill the device unless the pass has no more blocks to cut
    CHECK(n_list * runs >= 8 * lanes || R == 1 || n_list * (uint64_t)probe_adaptive_runs(nb, R - 1) >= 8 * lanes || runs == nb);
    const uint64_t per = probe_adaptive_range_positions(n_list, nb, R, cap), nr = radiance_n_ranges(n_list, per);
    CHECK(per >= 1 && per <= n_list);
    uint64_t next = 0;
    for (uint64_t r = 0; r < nr; r++) {
        const RadianceRange g = radiance_range(n_list, per, r);
        CHECK(g.first == next && g.count >= 1 && g.count <= per);
        const uint64_t units = g.count * runs;
        CHECK(units >= 1 && units <= kBig);
        CHECK(g.count == 1 || probe_adaptive_slab_bytes(g.count, nb) <= cap);
        CHECK(probe_adaptive_slab_bytes(g.count, nb) == g.count * nb * 16ull);
        const uint64_t grid = std::min<uint64_t>((units + 255) / 256, lanes / 256 ? lanes / 256 : 1);
        const uint32_t J = probe_adaptive_job_units(R, units, grid * 4);
        CHECK(J >= 64 && J % 64 == 0 && J <= 64 * 32);
        const uint64_t jobs = radiance_n_jobs(units, J);
        CHECK(jobs >= 1 && jobs <= kBig && (jobs - 1) * J < units && jobs * J >= units);
        CHECK((jobs - 1) * J + J <= 0xffffffffull);  // a job's end, taken before the clamp to n_units, fits 32 bits
        next = g.first + g.count;
        if (nr > 64 && r == 31) {  // (a long cut: the first ranges, then the tail)
            r = nr - 33;
            next = radiance_range(n_list, per, r + 1).first;
        }
    }
    CHECK(next == n_list);
    CHECK(radiance_range(n_list, per, nr).count == 0);
}

static void schedule(int min_spp, int step_spp, int cap) {
    std::vector<int> cps;
    CHECK(adaptive_checkpoints(min_spp, step_spp, cap, 0.02f, 0, cps) == nullptr);
    CHECK(!cps.empty() && cps.front() == min_spp && cps.back() == cap);
    const uint64_t lanes = 256ull * 8 * 256;
    int prev = 0;
    uint32_t blocks = 0;
    for (int n_k : cps) {
        CHECK(probe_adaptive_first_block(prev) == blocks);
        blocks += probe_adaptive_pass_blocks(prev, n_k);
        for (uint64_t n_list : {1ull, 47ull, 96ull, 5003ull, 262144ull, kBig}) {
            pass(n_list, prev, n_k, lanes, 1ull << 30);
            pass(n_list, prev, n_k, lanes, 700 * 2 * 16);
            pass(n_list, prev, n_k, lanes, 8);  // a cap below one position's row: one position per range
            pass(n_list, prev, n_k, 256, 1ull << 62);
        }
        prev = n_k;
    }
    CHECK(blocks * RTW_SUM_BLOCK == (uint32_t)cap);  // the passes tile [0, cap)
}

int main() {
    schedule(64, 0, 4096);
    schedule(32, 48, 272);
    schedule(32, 0, 256);
    // sample_offset moves neither the blocks nor the units of a pass: both are counted from it (0 and 16 give the same plan)
    {
        std::vector<int> cps;
        CHECK(adaptive_checkpoints(32, 48, 272, 0.0f, 0, cps) == nullptr);
        const int want[] = {32, 80, 128, 176, 224, 272};
        CHECK(cps.size() == 6);
        for (size_t k = 0; k < cps.size() && k < 6; k++) CHECK(cps[k] == want[k]);
        for (int off : {0, 16}) {
            (void)off;
            CHECK(probe_adaptive_first_block(128) == 8 && (probe_adaptive_first_block(128) % RTW_SUM_UNIT_BLOCKS) == 0);  // a pass that starts a unit
            CHECK(probe_adaptive_first_block(224) == 14 && probe_adaptive_pass_blocks(224, 272) == 3);                     // one that crosses into the next
        }
    }
    // R: few probes and a long pass are cut to single blocks; many probes take their pass in one run
    CHECK(probe_adaptive_run_blocks(31, 81, 524288) == 1);
    CHECK(probe_adaptive_run_blocks(kBig, 81, 524288) == 81);
    CHECK(probe_adaptive_run_blocks(524288ull * 8, 4, 524288) == 4 && probe_adaptive_run_blocks(524288ull * 4, 4, 524288) == 2);
    CHECK(probe_adaptive_run_blocks(1, 1, 0) == 1);
    // 2^31 - 1 probes: sizes in 64 bits
    CHECK(probe_adaptive_slab_bytes(kBig, 256) == kBig * 256 * 16);
    CHECK(probe_adaptive_slab_bytes(kBig, 1u << 27) == kBig * (1ull << 27) * 16);  // below 2^63
    CHECK(probe_adaptive_range_positions(kBig, 4, 4, 1ull << 62) == kBig && probe_adaptive_range_positions(kBig, 4, 1, 1ull << 62) == kBig / 4);
    CHECK(probe_adaptive_range_positions(kBig, 4, 4, 1ull << 30) == (1ull << 30) / 64);
    CHECK(probe_adaptive_range_positions(0, 4, 4, 1ull << 30) == 1);
    // the family's state (rtw_adaptive_plan.h), with and without the renderer's `part`: sections in order, 256-byte aligned, every
    // array inside the allocation, no section's offset smaller for more entries
    typedef AdaptiveLayout AL;
    const auto up = [](uint64_t b) { return (b + 255) & ~255ull; };
    for (const bool want_part : {false, true})
        for (uint64_t n : {1ull, 63ull, 64ull, 65ull, 96ull, 131075ull, kBig}) {
            const AL l = adaptive_layout(n, want_part);
            const uint64_t nw = (n + 63) / 64;
            uint64_t need[AL::kSections];
            need[AL::kAccum] = n * 16; need[AL::kUpart] = n * 16; need[AL::kPart] = want_part ? n * 16 : 0; need[AL::kMom] = n * 16;
            need[AL::kN] = n * 4; need[AL::kErr] = n * 4; need[AL::kTotal] = n * 4; need[AL::kList0] = n * 4 + 4; need[AL::kList1] = n * 4 + 4;
            need[AL::kMasks] = nw * 8; need[AL::kOffsets] = nw * 4;
            CHECK(l.off[0] == 0);
            for (int k = 0; k < AL::kSections; k++) CHECK(l.off[k] % 256 == 0 && l.off[k + 1] >= l.off[k] + need[k]);
            CHECK(l.off[AL::kPart + 1] - l.off[AL::kPart] == (want_part ? up(n * 16) : 0));  // a query's entry does not pay for `part`
            CHECK(l.bytes() == l.off[AL::kSections] && l.bytes() >= n * (want_part ? 84 : 68));
            const AL m = adaptive_layout(n + 1, want_part);
            for (int k = 0; k <= AL::kSections; k++) CHECK(m.off[k] >= l.off[k]);
            // without `part`: the bytes of the layout the probes had before the family shared it, section by section
            if (!want_part)
                CHECK(l.bytes() == 3 * up(n * 16) + 3 * up(n * 4) + 2 * up(n * 4 + 4) + up(nw * 8) + up(nw * 4));
            else
                CHECK(l.bytes() == adaptive_layout(n, false).bytes() + up(n * 16));
        }
    CHECK(adaptive_layout(1, false).bytes() == 10 * 256 && adaptive_layout(65, false).bytes() == 3 * 1280 + 3 * 512 + 2 * 512 + 2 * 256);
    CHECK(adaptive_layout(kBig, false).bytes() == 3 * 34359738368ull + 5 * 8589934592ull + 268435456ull + 134217728ull);
    if (fails) return 1;
    printf("probe_adaptive_plan_check ok\n");
    return 0;
}
