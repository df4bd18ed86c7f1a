// CPU check of rtw_views' planning (view_pixels_ok, view_pixels and view_pixel of raytracing_weekend_amd/csrc/rtw_radiance_plan.h, with
// magic_div of rtw_plan.h as the kernel applies it), compiled with g++ -fsanitize=address,undefined and run by
// tests/test_views_cpu.py: the split of a flattened pixel into (view, y, x) and its stream key, the same split through the
// multiply-high constants, ranges and chunks that begin and end inside a view, and the size limit in 64 bits. Prints
// "view_plan_check ok" and returns 0, or says what failed.
#include <cstdio>

#include "../../raytracing_weekend_amd/csrc/rtw_plan.h"
#include "../../raytracing_weekend_amd/csrc/rtw_radiance_plan.h"
using namespace rtwk;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

// fastdiv of rtw_kernels.h, restated: n / d with magic_div's constants
static uint32_t fastdiv(uint32_t n, uint32_t m, uint32_t s1, uint32_t s2) {
    const uint32_t t = (uint32_t)(((uint64_t)m * n) >> 32);
    return (t + ((n - t) >> s1)) >> s2;
}

// pixel p of a call of w x h frames, as the kernel splits it (first + ray = p), against view_pixel and against the definition
static void split(uint64_t p, int32_t w, int32_t h) {
    uint32_t fm, f1, f2, wm, w1, w2;
    magic_div((uint32_t)w * (uint32_t)h, fm, f1, f2);
    magic_div((uint32_t)w, wm, w1, w2);
    const uint32_t view = fastdiv((uint32_t)p, fm, f1, f2);
    const uint32_t key = (uint32_t)p - view * ((uint32_t)w * (uint32_t)h);
    const uint32_t y = fastdiv(key, wm, w1, w2), x = key - y * (uint32_t)w;
    const ViewPixel v = view_pixel(p, w, h);
    CHECK(v.view == view && v.y == y && v.x == x && v.key == key);
    CHECK(x < (uint32_t)w && y < (uint32_t)h && key == (uint32_t)w * y + x);
    CHECK(((uint64_t)view * (uint64_t)h + y) * (uint64_t)w + x == p);
}

static void frames(uint64_t n_views, int32_t w, int32_t h) {
    CHECK(view_pixels_ok(n_views, w, h));
    const uint64_t n = view_pixels(n_views, w, h), frame = (uint64_t)w * (uint64_t)h;
    CHECK(n == n_views * frame && n <= 0x7fffffffull);
    const uint64_t probe[] = {0, 1, (uint64_t)w - 1, (uint64_t)w, frame - 1, frame, frame + 1, n / 2, n - frame, n - (uint64_t)w, n - 2, n - 1};
    for (uint64_t p : probe)
        if (p < n) split(p, w, h);
    if (n <= 4096)
        for (uint64_t p = 0; p < n; p++) split(p, w, h);
}

// the ranges of a call under a slab cap, and chunks of `chunk` pixels cut into ranges again: consecutive, none empty, every pixel once;
// `mid` says that some range has to begin inside a view
static void cuts(uint64_t n_views, int32_t w, int32_t h, int32_t spp, uint64_t cap, uint64_t chunk, bool mid) {
    const uint64_t n = view_pixels(n_views, w, h), frame = (uint64_t)w * (uint64_t)h;
    uint64_t next = 0;
    bool saw_mid = false;
    for (uint64_t i0 = 0; i0 < n; i0 += chunk) {
        const uint64_t m = std::min(chunk, n - i0);
        const uint64_t per = radiance_range_rays(m, spp, cap), nr = radiance_n_ranges(m, per);
        for (uint64_t r = 0; r < nr; r++) {
            const RadianceRange g = radiance_range(m, per, r);
            CHECK(i0 + g.first == next && g.count >= 1);
            CHECK(radiance_units(spp) == 1 || g.count == 1 || radiance_slab_bytes(g.count, spp) <= cap);
            if ((i0 + g.first) % frame != 0) saw_mid = true;
            split(i0 + g.first, w, h);  // what the launch's first lane and its last one compute
            split(i0 + g.first + g.count - 1, w, h);
            next = i0 + g.first + g.count;
        }
    }
    CHECK(next == n && saw_mid == mid);
}

int main() {
    const uint64_t big = 0x7fffffffull;
    // the pixel split
    frames(3, 7, 5);
    frames(41, 7, 5);
    frames(3, 24, 16);
    frames(1, 1, 1);
    frames(5, 1, 1);
    frames(big, 1, 1);              // the limit, one pixel per view
    frames(1, (int32_t)big, 1);     // ... one row
    frames(1, 1, (int32_t)big);     // ... one column
    frames(2, 46340, 23170);        // 2 147 395 600 pixels
    frames(32767, 256, 256);        // 2^31 - 2^16
    frames(1, 46341, 46340);        // 2 147 441 940
    split(big - 1, 46341, 46340 + 1);  // (a frame need not be complete for the split to hold)
    // the size limit, in 64 bits
    CHECK(view_pixels_ok(0, 1, 1) && view_pixels_ok(0, INT32_MAX, INT32_MAX) && view_pixels(0, INT32_MAX, INT32_MAX) == 0);
    CHECK(view_pixels_ok(big, 1, 1) && !view_pixels_ok(big + 1, 1, 1));
    CHECK(view_pixels_ok(1, INT32_MAX, 1) && !view_pixels_ok(2, INT32_MAX, 1) && !view_pixels_ok(1, INT32_MAX, 2));
    CHECK(!view_pixels_ok(1, 65536, 32768) && view_pixels_ok(1, 65536, 32767) && !view_pixels_ok(1, INT32_MAX, INT32_MAX));
    CHECK(!view_pixels_ok(1ull << 33, 1, 1) && !view_pixels_ok(1ull << 62, 4, 1) && !view_pixels_ok(~0ull, 2, 2));  // products that wrap 64 bits
    CHECK(!view_pixels_ok((1ull << 32) + 1, 65536, 65536) && !view_pixels_ok(1ull << 32, INT32_MAX, INT32_MAX));
    CHECK(view_pixels_ok(32768, 256, 255) && !view_pixels_ok(32768, 256, 256));
    // ranges and chunks that cut a view
    cuts(3, 7, 5, 272, 50 * 3 * 16, big, true);    // 3 units per pixel, 50 pixels per range: 50, 50, 5 - the second begins in view 1
    cuts(3, 7, 5, 272, 16, big, true);             // a cap below one pixel's units: one pixel per range
    cuts(3, 7, 5, 16, 1 << 20, 50, true);          // chunks of 50 pixels
    cuts(3, 7, 5, 272, 20 * 3 * 16, 50, true);     // chunks of 50, cut into ranges of 20
    cuts(3, 7, 5, 272, 1 << 20, big, false);       // one range
    cuts(41, 7, 5, 144, 1 << 30, 35, false);       // a chunk per view
    cuts(1000, 24, 16, 129, 1 << 20, 100000, true);
    if (fails) return 1;
    printf("view_plan_check ok\n");
    return 0;
}
