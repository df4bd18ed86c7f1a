// CPU check of the planning of rtw_views_guides and rtw_denoise_views (raytracing_weekend_amd/csrc/rtw_view_guides_plan.h, with
// magic_div of rtw_plan.h as k_atrous_guided_views applies it), compiled with g++ -fsanitize=address,undefined and run by
// tests/test_views_guides_cpu.py: the staging of a chunk's requested guides, the chunk size, the split of a flattened pixel into its
// frame, row and column and the clamp of a tap inside that frame, the buffer a denoiser pass writes, and the scratch size. Prints
// "view_guides_plan_check ok" and returns 0, or says what failed.
#include <cstdio>

#include "../../raytracing_weekend_amd/csrc/rtw_plan.h"
#include "../../raytracing_weekend_amd/csrc/rtw_view_guides_plan.h"
using namespace rtwk;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

// fastdiv of rtw_kernels.h, restated: n / d with magic_div's constants
static uint32_t fastdiv(uint32_t n, uint32_t m, uint32_t s1, uint32_t s2) {
    const uint32_t t = (uint32_t)(((uint64_t)m * n) >> 32);
    return (t + ((n - t) >> s1)) >> s2;
}

// the staging of every subset of the four buffers: sections in the struct's order, aligned, disjoint, large enough, nothing for a
// buffer nobody wants
static void stage(uint64_t chunk) {
    for (int mask = 0; mask < 16; mask++) {
        const bool want[4] = {(mask & 1) != 0, (mask & 2) != 0, (mask & 4) != 0, (mask & 8) != 0};
        const ViewGuideStage s = view_guides_stage(chunk, want);
        uint64_t end = 0, sum = 0;
        for (int k = 0; k < 4; k++) {
            if (!want[k]) continue;
            CHECK(s.off[k] % 256 == 0 && s.off[k] >= end);
            end = s.off[k] + chunk * kGuideEntryBytes[k];
            sum += chunk * kGuideEntryBytes[k];
        }
        CHECK(end <= s.bytes && s.bytes % 256 == 0 && s.bytes >= sum && s.bytes < sum + 4 * 256);
        CHECK((mask == 0) == (s.bytes == 0));
    }
}

// pixel p of frames of w x h as the kernel splits it, against frame_pixel and the definition; every tap of every pass stays inside
// the pixel's frame and is the per-frame filter's tap
static void split(uint64_t p, int32_t w, int32_t h) {
    uint32_t fm, f1, f2;
    magic_div((uint32_t)w * (uint32_t)h, fm, f1, f2);
    const uint32_t frame = (uint32_t)w * (uint32_t)h;
    const uint32_t view = fastdiv((uint32_t)p, fm, f1, f2), base = view * frame;
    const int q = (int)((uint32_t)p - base), y = q / w, x = q - y * w;
    const FramePixel f = frame_pixel(p, w, h);
    CHECK(f.base == base && f.y == y && f.x == x && x >= 0 && x < w && y >= 0 && y < h);
    CHECK(f.base % frame == 0 && f.base + (uint64_t)y * (uint64_t)w + (uint64_t)x == p);
    for (int it = 0; it < 8; it++) {
        const int step = 1 << it;
        for (int dy = -2; dy <= 2; dy++)
            for (int dx = -2; dx <= 2; dx++) {
                // the kernel's statements
                int yy = y + dy * step;
                yy = yy < 0 ? 0 : (yy > h - 1 ? h - 1 : yy);
                int xx = x + dx * step;
                xx = xx < 0 ? 0 : (xx > w - 1 ? w - 1 : xx);
                const uint32_t j = base + (uint32_t)(yy * w + xx);
                CHECK(j == frame_tap(f, w, h, dx, dy, step));
                CHECK(j >= base && j - base < frame);                      // inside the pixel's own frame
                CHECK(j - base == (uint32_t)yy * (uint32_t)w + (uint32_t)xx);  // k_atrous_guided's index in that frame alone
            }
    }
}

static void frames(uint64_t n_views, int32_t w, int32_t h) {
    CHECK(view_pixels_ok(n_views, w, h));
    const uint64_t n = view_pixels(n_views, w, h), frame = (uint64_t)w * (uint64_t)h;
    const uint64_t probe[] = {0, 1, (uint64_t)w - 1, (uint64_t)w, frame - 1, frame, frame + 1, n / 2, n - frame, n - (uint64_t)w, n - 2, n - 1};
    for (uint64_t p : probe)
        if (p < n) split(p, w, h);
    if (n <= 4096)
        for (uint64_t p = 0; p < n; p++) split(p, w, h);
}

int main() {
    const uint64_t big = 0x7fffffffull;
    const uint64_t chunks[] = {1, 15, 16, 50, 64, 105, 1ull << 20, big};
    for (uint64_t chunk : chunks) stage(chunk);
    {   // all four of a 50-pixel chunk: 800 -> 1024, 800 -> 1024, 200 -> 256, 200 -> 256
        const bool all[4] = {true, true, true, true}, dp[4] = {false, false, true, true};
        const ViewGuideStage s = view_guides_stage(50, all), t = view_guides_stage(50, dp);
        CHECK(s.off[0] == 0 && s.off[1] == 1024 && s.off[2] == 2048 && s.off[3] == 2304 && s.bytes == 2560);
        CHECK(t.off[2] == 0 && t.off[3] == 256 && t.bytes == 512);
    }
    CHECK(view_guides_chunk(105, 1u << 20) == 105 && view_guides_chunk(105, 50) == 50 && view_guides_chunk(105, 1) == 1);
    CHECK(view_guides_chunk(105, 0) == 1 && view_guides_chunk(big, big) == big && view_guides_chunk(1, big) == 1);
    // the frame split and the taps
    frames(3, 7, 5);
    frames(41, 7, 5);
    frames(3, 24, 16);   // hole size 16 at pass 4 exceeds the 16 rows
    frames(1, 1, 1);
    frames(5, 1, 1);
    frames(7, 1, 9);
    frames(7, 9, 1);
    frames(big, 1, 1);
    frames(7, 1 << 28, 1);    // the largest frame (rtw_denoise_guided's limit), one row: x + 2 * 128 stays an int
    frames(7, 1, 1 << 28);    // ... one column
    frames(7, 16384, 16384);
    frames(32767, 256, 256);  // 2^31 - 2^16 pixels
    CHECK(denoise_views_frame_ok(1, 1) && denoise_views_frame_ok(1 << 28, 1) && denoise_views_frame_ok(16384, 16384));
    CHECK(!denoise_views_frame_ok((1 << 28) + 1, 1) && !denoise_views_frame_ok(16385, 16384) && !denoise_views_frame_ok(INT32_MAX, INT32_MAX));
    // the passes: the last one writes the output, consecutive passes alternate, so no pass reads the buffer it writes
    for (int n = 1; n <= 8; n++) {
        CHECK(denoise_views_writes_output(n, n - 1));
        for (int it = 1; it < n; it++) CHECK(denoise_views_writes_output(n, it) != denoise_views_writes_output(n, it - 1));
    }
    CHECK(denoise_views_writes_output(1, 0) && !denoise_views_writes_output(2, 0) && denoise_views_writes_output(5, 0));
    // the scratch: one buffer beside the output for more than one pass, the host entry's four copies, in 64 bits
    CHECK(denoise_views_buffer_bytes(1) == 256 && denoise_views_buffer_bytes(16) == 256 && denoise_views_buffer_bytes(17) == 512);
    CHECK(denoise_views_scratch_bytes(105, 1, false) == 0 && denoise_views_scratch_bytes(105, 2, false) == 1792);
    CHECK(denoise_views_scratch_bytes(105, 1, true) == 4 * 1792 && denoise_views_scratch_bytes(105, 5, true) == 5 * 1792);
    CHECK(denoise_views_buffer_bytes(big) == 34359738368ull && denoise_views_scratch_bytes(big, 8, true) == 5 * 34359738368ull);
    if (fails) return 1;
    printf("view_guides_plan_check ok\n");
    return 0;
}
