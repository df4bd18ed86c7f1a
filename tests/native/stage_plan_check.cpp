// CPU check of the staging slab's layout (raytracing_weekend_amd/csrc/rtw_stage_plan.h stage_plan, and view_guides_stage of
// rtw_view_guides_plan.h, which is made of it), compiled with g++ -fsanitize=address,undefined and run by tests/test_stage_cpu.py.
// Over the section lists of every host variant of the query family, chunks from 1 to 2^31 - 1 and every subset of wanted sections:
// offsets 256-byte aligned and ascending, sections disjoint and inside `bytes`, nothing for a section nobody wants, no 64-bit
// overflow, and every section - hence the slab - at least as large as the entry points made it before they shared this function
// (those formulas are restated below). Prints "stage_plan_check ok" and returns 0, or says what failed.
#include <cstdio>

#include "../../raytracing_weekend_amd/csrc/rtw_stage_plan.h"
#include "../../raytracing_weekend_amd/csrc/rtw_view_guides_plan.h"
using namespace rtwk;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

typedef unsigned __int128 u128;
static uint64_t al(uint64_t b) { return (b + 255) & ~(uint64_t)255; }

// A family's sections and what each took before: every section rounded up to 256 bytes, except that the families which computed
// their offsets inline left the last one as it was (nothing followed it).
struct Family {
    const char* name;
    int n;
    uint64_t width[kStageMaxSections];
    bool last_unaligned;
};
static const Family kFamilies[] = {
    {"cast", 8, {32, 4, 4, 4, 4, 4, 16, 8}, false},     // ray, ray_time, gather_time, t, prim, material, normal, uv
    {"radiance", 2, {32, 16}, true},                    // ray, result (stride 1: rtw_radiance, rtw_probe)
    {"probe_sh", 2, {32, 16 * 9}, true},                // point, nine float4
    {"views", 1, {16}, true},                           // result
    {"probe_adaptive", 4, {32, 16, 4, 4}, true},        // probe, rgba, spp, err
    {"views_adaptive", 3, {16, 4, 4}, true},            // rgba, spp, err
    {"views_guides", 4, {16, 16, 4, 4}, false},         // albedo, normal, depth, prim (view_guides_stage)
};
static uint64_t before(const Family& f, int k, uint64_t chunk) { return f.last_unaligned && k == f.n - 1 ? chunk * f.width[k] : al(chunk * f.width[k]); }

// the whole slab of a call before, as the entry points wrote it
static uint64_t before_whole(const Family& f, uint64_t chunk) {
    const uint64_t c = chunk;
    switch (f.n) {
    case 8: {  // impl_cast: all eight sections whatever the caller wanted
        uint64_t bytes = 0;
        for (int k = 0; k < 8; k++) bytes += (c * f.width[k] + 255) & ~(uint64_t)255;
        return bytes;
    }
    case 2: return ((c * 32 + 255) & ~(uint64_t)255) + c * f.width[1];  // query_host: rays_bytes + chunk * 16 * stride
    case 1: return c * 16;                                               // impl_views
    case 3: return al(c * 16) + al(c * 4) + c * 4;                       // impl_adaptive_views: o_err + chunk * 4
    default:
        if (f.last_unaligned) return al(c * 32) + al(c * 16) + al(c * 4) + c * 4;  // impl_adaptive_probe: o_err + chunk * 4
        return al(c * 16) + al(c * 16) + al(c * 4) + al(c * 4);                    // view_guides_stage, all four
    }
}

static void check(const Family& f, uint64_t chunk) {
    for (unsigned mask = 0; mask < (1u << f.n); mask++) {
        bool want[kStageMaxSections];
        for (int k = 0; k < kStageMaxSections; k++) want[k] = (mask >> k) & 1u;
        const StagePlan s = stage_plan(chunk, f.n, f.width, want);
        uint64_t end = 0, sum_before = 0;
        u128 exact = 0;  // the same sum in 128 bits: nothing wrapped
        int prev = -1;
        for (int k = 0; k < f.n; k++) {
            if (!want[k]) {
                CHECK(s.off[k] == end);  // it takes no space: the next section begins where this one would have
                continue;
            }
            CHECK(s.off[k] % 256 == 0 && s.off[k] >= end);
            CHECK(prev < 0 || s.off[k] > s.off[prev]);  // ascending, disjoint: it begins where the one before ends
            const uint64_t size = al(chunk * f.width[k]);
            CHECK(size >= chunk * f.width[k] && size >= before(f, k, chunk));
            end = s.off[k] + size;
            sum_before += before(f, k, chunk);
            exact += ((u128)chunk * f.width[k] + 255) / 256 * 256;
            prev = k;
        }
        CHECK(end == s.bytes && (u128)s.bytes == exact && s.bytes % 256 == 0);
        CHECK(s.bytes >= sum_before);
        CHECK((mask == 0) == (s.bytes == 0));
        if (mask + 1 == (1u << f.n)) CHECK(s.bytes >= before_whole(f, chunk) && before_whole(f, chunk) >= sum_before);
        for (int k = f.n; k < kStageMaxSections; k++) CHECK(s.off[k] == 0);
        if (f.n == 4 && !f.last_unaligned) {  // the guides' own function is this one
            const ViewGuideStage g = view_guides_stage(chunk, want);
            CHECK(g.bytes == s.bytes);
            for (int k = 0; k < 4; k++) CHECK(g.off[k] == s.off[k] && f.width[k] == kGuideEntryBytes[k]);
        }
    }
}

int main() {
    const uint64_t chunks[] = {1, 2, 15, 16, 17, 255, 256, 257, 1ull << 20, 0x7fffffffull};
    for (const Family& f : kFamilies)
        for (uint64_t chunk : chunks) check(f, chunk);
    {   // by hand: a cast of 100 rays that wants only uv (3200 -> 3328 of rays, 800 -> 1024 of uv), and all of it
        const uint64_t w[8] = {32, 4, 4, 4, 4, 4, 16, 8};
        const bool uv[8] = {true, false, false, false, false, false, false, true};
        const bool all[8] = {true, true, true, true, true, true, true, true};
        const StagePlan s = stage_plan(100, 8, w, uv), t = stage_plan(100, 8, w, all);
        CHECK(s.off[0] == 0 && s.off[7] == 3328 && s.bytes == 4352);
        CHECK(t.off[1] == 3328 && t.off[2] == 3840 && t.off[6] == 5888 && t.off[7] == 7680 && t.bytes == 8704);
        // a smaller chunk of a later call lies where its own size says, not where the larger call's sections were
        CHECK(stage_plan(10, 8, w, all).off[7] == 512 + 5 * 256 + 256 && stage_plan(10, 8, w, all).bytes == 2304);
    }
    {   // 37 rays of rtw_radiance, 5 points of rtw_probe_sh
        const uint64_t r[2] = {32, 16}, sh[2] = {32, 144};
        const bool both[2] = {true, true};
        CHECK(stage_plan(37, 2, r, both).off[1] == 1280 && stage_plan(37, 2, r, both).bytes == 1280 + 768);
        CHECK(stage_plan(5, 2, sh, both).off[1] == 256 && stage_plan(5, 2, sh, both).bytes == 256 + 768);
    }
    if (fails) return 1;
    printf("stage_plan_check ok\n");
    return 0;
}
