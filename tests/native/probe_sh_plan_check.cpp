// CPU check of rtw_probe_sh's planning (the 144-bytes-per-unit functions of raytracing_weekend_amd/csrc/rtw_radiance_plan.h), compiled
// with g++ -fsanitize=address,undefined and run by tests/test_probe_sh_cpu.py: the slab size in 64 bits, the cut of a batch into
// point ranges under a cap, and the bound that keeps a launch's float4 indices below 2^31. Prints "probe_sh_plan_check ok" and
// returns 0, or says what failed.
#include <cstdio>

#include "../../raytracing_weekend_amd/csrc/rtw_radiance_plan.h"
using namespace rtwk;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

// the ranges of (n, spp, cap) tile [0, n): consecutive, none empty, no point twice, each within the cap (unless it is one point) and
// with every float4 index (unit * count + point) * 9 + j below 2^31
static void tiles(uint64_t n, int32_t spp, uint64_t cap, uint64_t want_ranges) {
    const uint64_t per = probe_sh_range_points(n, spp, cap), nr = radiance_n_ranges(n, per), u = radiance_units(spp);
    CHECK(per >= 1 && nr == want_ranges);
    uint64_t next = 0;
    for (uint64_t r = 0; r < nr; r++) {
        const RadianceRange g = radiance_range(n, per, r);
        CHECK(g.first == next && g.count >= 1 && g.count <= per);
        CHECK(g.count * u <= kProbeShMaxLaunchUnits && g.count * u * 9 <= 0x7fffffffull);
        CHECK(u == 1 || g.count == 1 || probe_sh_slab_bytes(g.count, spp) <= cap);
        next = g.first + g.count;
    }
    CHECK(next == n);
    CHECK(radiance_range(n, per, nr).count == 0);
}

int main() {
    const uint64_t big = 0x7fffffffull;
    CHECK(kProbeShUnitBytes == 144 && kProbeShMaxLaunchUnits == big / 9 && kProbeShMaxLaunchUnits * 9 <= big);
    // slab bytes in 64 bits
    CHECK(probe_sh_slab_bytes(big, 128) == 0 && probe_sh_slab_bytes(5, 1) == 0);
    CHECK(probe_sh_slab_bytes(big, 129) == big * 2 * 144 && probe_sh_slab_bytes(80, 272) == 80 * 3 * 144);
    CHECK(probe_sh_slab_bytes(big, INT32_MAX) == big * (1ull << 24) * 144);  // below 2^63: no wrap
    CHECK(probe_sh_slab_bytes(262144, 1024) == 262144ull * 8 * 144);
    // point ranges
    tiles(1, 1, 1 << 20, 1);
    tiles(big, 1, 16, 10);                        // one unit per point: no slab, but nine float4 each: ten launches
    tiles(big, 129, 1ull << 62, 19);              // the 2^31 bound at spp 129: (2^31 - 1) / 18 points per range
    tiles(big, 1 << 20, 1ull << 62, 73729);       // and at spp 2^20: 8192 units per point, 29 127 points per range
    tiles(big, 129, 1ull << 30, 577);             // the cap: 2^30 / 288 points per range
    tiles(96, 272, 40 * 3 * 144, 3);              // 40 points per range: 40, 40, 16
    tiles(5003, 272, 432 * 1000, 6);
    tiles(7, 272, 16, 7);                         // a cap below one point's units: one point per range
    tiles(9, INT32_MAX, 1ull << 62, 1);
    tiles(200, INT32_MAX, 1ull << 62, 15);        // 2^24 units per point: 14 points per range
    CHECK(probe_sh_range_points(big, 129, 1ull << 62) == big / 9 / 2);
    CHECK(probe_sh_range_points(big, 1 << 20, 1ull << 62) == big / 9 / 8192);
    CHECK(probe_sh_range_points(0, 129, 1 << 20) == 1);
    if (fails) return 1;
    printf("probe_sh_plan_check ok\n");
    return 0;
}
