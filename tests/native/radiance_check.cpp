// CPU check of rtw_radiance's planning (raytracing_weekend_amd/csrc/rtw_radiance_plan.h), compiled with
// g++ -fsanitize=address,undefined and run by tests/test_radiance_cpu.py: units per ray, the slab size in 64 bits, the cut of a
// batch into ray ranges under a cap, stream keys that wrap, and the job size. Prints "radiance_check ok" and returns 0, or says
// what failed.
#include <cstdio>
#include <vector>

#include "../../raytracing_weekend_amd/csrc/rtw_radiance_plan.h"
using namespace rtwk;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

// the ranges of (n, spp, cap) tile [0, n): consecutive, none empty, no ray twice, each within the cap and the launch limit
static void tiles(uint64_t n, int32_t spp, uint64_t cap, uint64_t want_ranges) {
    const uint64_t per = radiance_range_rays(n, spp, cap), nr = radiance_n_ranges(n, per), u = radiance_units(spp);
    CHECK(per >= 1 && nr == want_ranges);
    uint64_t next = 0;
    for (uint64_t r = 0; r < nr; r++) {
        const RadianceRange g = radiance_range(n, per, r);
        CHECK(g.first == next && g.count >= 1 && g.count <= per);
        CHECK(g.count * u <= kRadianceMaxLaunchUnits);
        CHECK(u == 1 || g.count == 1 || radiance_slab_bytes(g.count, spp) <= cap);
        next = g.first + g.count;
    }
    CHECK(next == n);
    CHECK(radiance_range(n, per, nr).count == 0);
}

int main() {
    // units per ray
    CHECK(kRadianceUnit == 128);
    CHECK(radiance_units(1) == 1 && radiance_units(16) == 1 && radiance_units(128) == 1 && radiance_units(129) == 2 && radiance_units(272) == 3);
    CHECK(radiance_units(INT32_MAX) == (1u << 24));
    // slab bytes in 64 bits
    const uint64_t big = 0x7fffffffull;
    CHECK(radiance_slab_bytes(big, 128) == 0 && radiance_slab_bytes(5, 1) == 0);
    CHECK(radiance_slab_bytes(big, 129) == big * 2 * 16 && radiance_slab_bytes(big, 129) > (1ull << 35));
    CHECK(radiance_slab_bytes(big, INT32_MAX) == big * (1ull << 24) * 16);  // 2^59: no wrap
    CHECK(radiance_slab_bytes(80, 272) == 80 * 3 * 16);
    // ray ranges
    tiles(1, 1, 1 << 20, 1);
    tiles(big, 1, 16, 1);                       // one unit per ray: no slab, one launch of 2^31 - 1 units
    tiles(big, 129, 1ull << 30, 64);            // 2^25 rays per range
    tiles(5003, 272, 48 * 1000, 6);             // 1000 rays per range, the last one 3
    tiles(5000, 272, 48 * 1000, 5);
    tiles(7, 272, 16, 7);                       // a cap below one ray's units: one ray per range
    tiles(9, INT32_MAX, 1ull << 30, 3);         // 2^24 units per ray, 2^28 bytes: four rays per range
    tiles(1000, 1280, 1ull << 40, 1);
    CHECK(radiance_range_rays(big, 129, 1ull << 62) == big / 2);  // the launch limit, not the cap
    // keys wrap modulo 2^32
    const uint32_t k0 = 0xfffffffdu;  // 2^32 - 3
    CHECK(radiance_key(k0, 0) == k0 && radiance_key(k0, 2) == 0xffffffffu && radiance_key(k0, 3) == 0u && radiance_key(k0, 7) == 4u);
    CHECK(radiance_key(5, 1000) == 1005u && radiance_key(k0, big) == (uint32_t)(0xfffffffdull + big));
    {   // chunks of 3 rays carry the keys of an unchunked call
        std::vector<uint32_t> keys;
        for (uint64_t i0 = 0; i0 < 8; i0 += 3)
            for (uint64_t i = 0; i < 3 && i0 + i < 8; i++) keys.push_back(radiance_key(k0, i0) + (uint32_t)i);
        for (uint64_t i = 0; i < 8; i++) CHECK(keys[i] == (uint32_t)(k0 + i));
    }
    // jobs: a multiple of 64 units, at least one, all units covered, the queue rate bound of the header's comment
    for (int32_t spp : {1, 16, 48, 128, 129, 1024}) {
        for (uint64_t n_units : {1ull, 96ull, 524291ull, 16588800ull, 0x7fffffffull}) {
            const uint32_t ju = radiance_job_units(spp, n_units, 6144);
            const uint64_t nj = radiance_n_jobs(n_units, ju);
            CHECK(ju >= 64 && ju % 64 == 0 && ju <= 64 * 512);
            CHECK(nj * ju >= n_units && (nj - 1) * ju < n_units && nj <= 0xffffffffull);
            CHECK((uint64_t)(nj - 1) * ju + ju <= 0xffffffffull);  // job starts and ends fit 32 bits
        }
        CHECK(radiance_job_units(spp, 0x7fffffffull, 6144) * (uint64_t)std::min(spp, 128) >= 32768);
    }
    CHECK(radiance_job_units(1024, 16588800, 6144) == 256 && radiance_job_units(1, 96, 6144) == 64);
    if (fails) return 1;
    printf("radiance_check ok\n");
    return 0;
}
