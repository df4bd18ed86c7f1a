// CPU check of rtw_views_adaptive's planning (raytracing_weekend_amd/csrc/rtw_view_adaptive_plan.h), compiled with
// g++ -fsanitize=address,undefined and run by tests/test_views_adaptive_cpu.py: the tap of the dilated stop rule stays inside the
// pixel's own view and is the clamped pixel of that view (exhaustively on small shapes, and near 2^31 - 1 pixels), the batches of the
// host entry are whole views that tile the call for chunk values of 1, a frame exactly and beyond (and are what the entry's loop
// over uniform chunks of view_adaptive_chunk pixels visits), and a pass over the pixels of a
// batch is a pass rtw_probe_adaptive's plan can number. Prints "view_adaptive_plan_check ok" and returns 0, or says what failed.
#include <cstdio>
#include <vector>

#include "../../raytracing_weekend_amd/csrc/rtw_plan.h"
#include "../../raytracing_weekend_amd/csrc/rtw_view_adaptive_plan.h"
using namespace rtwk;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static const unsigned long long kBig = 0x7fffffffull;

static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// every pixel and every tap of n_views frames of w x h, against the definition written out with loops over (view, y, x)
static void taps(int n_views, int w, int h) {
    const uint64_t frame = (uint64_t)w * h;
    std::vector<int> seen(n_views * frame, 0);
    for (int v = 0; v < n_views; v++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const uint64_t p = ((uint64_t)v * h + y) * w + x;  // rtw_views' layout
                const ViewPixel vp = view_pixel(p, w, h);
                CHECK(vp.view == (uint64_t)v && vp.y == (uint32_t)y && vp.x == (uint32_t)x && vp.key == (uint32_t)(w * y + x));
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const uint64_t q = view_adaptive_neighbour(p, w, h, dx, dy);
                        const uint64_t want = (uint64_t)v * frame + (uint64_t)clampi(y + dy, 0, h - 1) * w + (uint64_t)clampi(x + dx, 0, w - 1);
                        CHECK(q == want);
                        CHECK(q >= (uint64_t)v * frame && q < (uint64_t)(v + 1) * frame);  // never another view
                        CHECK(q < (uint64_t)n_views * frame);
                        if (dx == 0 && dy == 0) CHECK(q == p);
                        // one view: the frame's own index, which is how rtw_render_adaptive runs k_adapt_decide (its shard: height = rows)
                        if (n_views == 1) CHECK(q == (uint64_t)clampi(y + dy, 0, h - 1) * w + (uint64_t)clampi(x + dx, 0, w - 1));
                    }
                seen[p]++;
            }
    for (int s : seen) CHECK(s == 1);
}

// the cut of n_views views of w x h under a chunk knob: whole views, in order, none empty, all of them
static void batches(uint64_t n_views, int w, int h, uint64_t chunk) {
    const uint64_t frame = (uint64_t)w * h;
    const uint64_t per = view_adaptive_batch_views(w, h, chunk);
    CHECK(per >= 1);
    CHECK(per == 1 || per * frame <= chunk);         // a batch holds at most `chunk` pixels unless one frame is already more
    CHECK(chunk / frame <= per);                     // and as many whole views as fit (by division: chunk may be 2^64 - 1)
    const uint64_t eff = std::min<uint64_t>(per, std::max<uint64_t>(n_views, 1)), nb = view_adaptive_n_batches(n_views, eff);
    uint64_t next = 0;
    for (uint64_t b = 0; b < nb; b++) {
        const RadianceRange g = view_adaptive_batch(n_views, eff, b);
        CHECK(g.first == next && g.count >= 1 && g.count <= eff);
        CHECK(view_pixels_ok(g.count, w, h));
        {   // the host entry's loop: uniform chunks of view_adaptive_chunk pixels over the call's n pixels are these views
            const uint64_t n = n_views * frame, chunk = view_adaptive_chunk(eff, w, h), i0 = b * chunk, m = std::min<uint64_t>(chunk, n - i0);
            CHECK(chunk == eff * frame && i0 < n && (i0 + chunk >= n) == (b + 1 == nb));
            CHECK(i0 % frame == 0 && m % frame == 0 && i0 / frame == g.first && m / frame == g.count);
        }
        next = g.first + g.count;
        if (nb > 64 && b == 31) {  // (a long cut: the first batches, then the tail)
            b = nb - 33;
            next = view_adaptive_batch(n_views, eff, b + 1).first;
        }
    }
    CHECK(next == n_views);
    CHECK(view_adaptive_batch(n_views, eff, nb).count == 0);
}

int main() {
    // small shapes, exhaustively: 1..3 views of 1x1, 1xN, Nx1 and 7x5 (35 pixels: a wave of 64 spans two views)
    for (int n = 1; n <= 3; n++) {
        taps(n, 1, 1);
        for (int k : {2, 3, 9, 64, 65}) { taps(n, 1, k); taps(n, k, 1); }
        taps(n, 7, 5);
        taps(n, 5, 7);
        taps(n, 24, 16);
    }
    // near 2^31 - 1 pixels: the last pixels of the last view, in 64 bits
    {
        struct { int w, h; } shapes[] = {{1, 1}, {7, 5}, {46340, 46340}, {32768, 65535}, {1, 0x7fffffff}, {0x7fffffff, 1}, {32, 32}};
        for (auto s : shapes) {
            const uint64_t frame = (uint64_t)s.w * s.h, n_views = kBig / frame, n = n_views * frame;
            CHECK(view_pixels_ok(n_views, s.w, s.h) && !view_pixels_ok(n_views + 1, s.w, s.h));
            CHECK(n <= kBig && n + frame > kBig);
            for (uint64_t p : std::vector<uint64_t>{n - 1, n - (uint64_t)s.w, n - frame, 0, frame - 1}) {
                if (p >= n) continue;
                const ViewPixel vp = view_pixel(p, s.w, s.h);
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const uint64_t q = view_adaptive_neighbour(p, s.w, s.h, dx, dy);
                        CHECK(q / frame == vp.view && q < n);
                        const ViewPixel vq = view_pixel(q, s.w, s.h);
                        CHECK(vq.y == (uint32_t)clampi((int)std::min<int64_t>((int64_t)vp.y + dy, 0x7fffffff), 0, s.h - 1));
                        CHECK(vq.x == (uint32_t)clampi((int)std::min<int64_t>((int64_t)vp.x + dx, 0x7fffffff), 0, s.w - 1));
                    }
            }
        }
    }
    // the batch cut: chunk 1 (one view per batch), a frame exactly, frames exactly, between, oversize, the knob's default
    for (auto s : {std::pair<int, int>{1, 1}, {7, 5}, {24, 16}, {32, 32}, {512, 512}}) {
        const uint64_t frame = (uint64_t)s.first * s.second;
        for (uint64_t n_views : {1ull, 2ull, 3ull, 41ull, 1536ull, kBig / frame}) {
            for (uint64_t chunk : std::vector<uint64_t>{1, frame - 1, frame, frame + 1, 2 * frame - 1, 2 * frame, 3 * frame, 50, 1ull << 20, 1ull << 22, kBig, ~0ull})
                if (chunk >= 1) batches(n_views, s.first, s.second, chunk);
        }
        CHECK(view_adaptive_batch_views(s.first, s.second, 1) == 1);
        CHECK(view_adaptive_batch_views(s.first, s.second, frame) == 1 && view_adaptive_batch_views(s.first, s.second, 2 * frame) == 2);
        CHECK(view_adaptive_batch_views(s.first, s.second, 3 * frame - 1) == 2);
    }
    CHECK(view_adaptive_batch_views(7, 5, 50) == 1 && view_adaptive_batch_views(7, 5, 70) == 2 && view_adaptive_batch_views(24, 16, 50) == 1);
    CHECK(view_adaptive_batch_views(0x7fffffff, 1, ~0ull) == (~0ull) / kBig);
    // a pass over a batch's pixels is one rtw_probe_adaptive's plan numbers: units below 2^31, ranges that tile the list
    {
        std::vector<int> cps;
        CHECK(adaptive_checkpoints(32, 48, 272, 0.02f, 1, cps) == nullptr);
        int prev = 0;
        for (int n_k : cps) {
            const uint32_t nb = probe_adaptive_pass_blocks(prev, n_k);
            for (uint64_t n_list : {1ull, 35ull, 105ull, 384ull * 3, 1536ull * 1024, kBig}) {
                for (uint64_t cap : {16ull, 1ull << 30}) {
                    const uint32_t R = probe_adaptive_run_blocks(n_list, nb, 256ull * 8 * 256);
                    const uint64_t per = probe_adaptive_range_positions(n_list, nb, R, cap);
                    CHECK(per >= 1 && per * probe_adaptive_runs(nb, R) <= kBig);
                    CHECK(cap != 16 || per == 1);  // a cap of one entry: one list position per range
                    const RadianceRange last = radiance_range(n_list, per, radiance_n_ranges(n_list, per) - 1);
                    CHECK(last.first + last.count == n_list && last.count >= 1);
                }
            }
            prev = n_k;
        }
        const AdaptiveLayout l = adaptive_layout(kBig, false);  // the per-pixel state of the largest call
        CHECK(l.bytes() >= kBig * 68);
    }
    if (fails) return 1;
    printf("view_adaptive_plan_check ok\n");
    return 0;
}
